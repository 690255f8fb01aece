/*
 * artp_c.h -- C ABI of libartp.so: the MI355X (gfx950) implementation of art_planner's
 * sampling + validity + edge hot path.
 *
 * This is the drop-in boundary.  The reference has no C/FFI seam for this path; its
 * seams are C++ virtuals.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference tree); art_planner_amd/host/ holds the C++ classes with the
 * reference's names/signatures that forward to these calls.
 *
 * Conventions
 *   - opaque context per device; all entry points return 0 (ARTP_OK) or a negative artp_status and
 *     never throw; calls on one context are serialised internally (one recursive lock held for the whole
 *     call, staging buffers included), contexts are independent.
 *   - plain pointers and sizes only.  Pointers are HOST memory unless the function name ends in
 *     `_dev`, in which case every buffer argument is DEVICE memory on the context's GPU and the call
 *     is asynchronous on the context's stream (artp_set_stream / artp_synchronize).
 *   - states are OMPL SE3 states flattened as 7 doubles: x y z qx qy qz qw.
 *   - dPose is the reference's HeightMapBoxChecker::dPose: 16 floats = origin[4], rotation[12]
 *     (row-major 3x4), art_planner/include/art_planner/validity_checker/height_map_box_checker.h:20-25.
 *   - layers are grid_map::Matrix storage: float32, column-major, rows = size.x, cols = size.y.
 */
#ifndef ARTP_C_H
#define ARTP_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct artp_ctx artp_ctx;

typedef enum {
  ARTP_OK = 0,
  ARTP_ERR_INVALID_ARG = -1,
  ARTP_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture: the product has NO CPU fallback */
  ARTP_ERR_HIP = -3,         /* a HIP runtime call failed; artp_last_error() has the text */
  ARTP_ERR_NO_MAP = -4,      /* a required layer was not uploaded (reference: hasMap() == false) */
  ARTP_ERR_CAPACITY = -5,    /* layer upload: a box window wider than 64 samples (diagonal / spacing + 4 > 64) does not
                                fit the LDS window tile; once a layer is accepted, no validity call returns it.  Also:
                                an output buffer too small (the planner calls below) */
  ARTP_ERR_NO_WEIGHTS = -6,
  ARTP_ERR_TIMEOUT = -7,     /* artp_group_synchronize: a member's stream did not finish in time */
  ARTP_ERR_COMM = -8,        /* RCCL missing, or a communicator call failed (artp_group_last_error) */
  ARTP_ERR_COST_FUNC = -9    /* the caller's motion-cost function (artp_cost_set_external_query) reported failure */
} artp_status;

/* Numeric fields of art_planner::Params the hot path reads
 * (art_planner/include/art_planner/params.h:14-123).  Angles in radians. */
typedef struct {
  double torso_length, torso_width, torso_height;   /* params.h:93-95  */
  double torso_off_x, torso_off_y, torso_off_z;     /* params.h:97-101 */
  double feet_off_x, feet_off_y, feet_off_z;        /* params.h:107-111 */
  double reach_x, reach_y, reach_z;                 /* params.h:113-117 */
  int unknown_space_untraversable;                  /* params.h:26 */
  double max_pitch_pert, max_roll_pert;             /* params.h:80-81 */
  int sample_from_distribution;                     /* params.h:81: 1 = samplePositionInMapFromDist (default),
                                                       0 = samplePositionInMap (uniform in the map) */
} artp_params;

void artp_params_defaults(artp_params* p);          /* params.h defaults */
void artp_params_yaml(artp_params* p);              /* art_planner_ros/config/params.yaml:55-71 */

const char* artp_status_string(int status);
const char* artp_last_error(const artp_ctx* ctx);
/* "gfx950" etc. of the context's device. */
const char* artp_device_arch(const artp_ctx* ctx);

/* Planner / StateValidityChecker construction (art_planner/src/planner.cpp:75-131,
 * validity_checker.cpp:9-15).  ARTP_ERR_INVALID_ARG, with *out = NULL and before any device is asked for: a torso or
 * reach size that is not finite or not positive, an offset that is not finite, a perturbation limit that is not finite
 * or negative (the sizes become window tiles and LDS sizes at the first upload).  Then ARTP_ERR_NO_DEVICE when there is
 * no GPU. */
int artp_create(int device, const artp_params* params, artp_ctx** out);
void artp_destroy(artp_ctx* ctx);
/* Run the context's work on a caller-provided hipStream_t (NULL = HIP's legacy default stream).
 * A fresh context uses a private non-blocking stream; artp_use_own_stream switches back to it. */
int artp_set_stream(artp_ctx* ctx, void* hip_stream);
int artp_use_own_stream(artp_ctx* ctx);
int artp_synchronize(artp_ctx* ctx); /* every lane's stream */

/* Lanes: a context owns up to 4 lanes, each with its own stream (artp_set_stream applies to the current lane) and
 * its own scratch buffers, queues and counters; the map, its tables and the sampler are shared.  Calls issued on
 * different lanes overlap on the GPU: a planner thread that validates a batch as two halves on two lanes hides the
 * pipeline's short serial kernels and pairs kernels with different bottlenecks (bench.py: 1.77 -> 1.66 ms per 2^22
 * states).  Every call works on the CURRENT lane (0 after artp_create); artp_set_lane switches it (first use of a
 * lane creates its stream).  Calls that only read the shared state are unordered across lanes.  Every call that WRITES
 * state the lanes share orders itself, on the device: the height layers and their tables (artp_upload_layer,
 * artp_update_layer_rect(s), artp_preprocessed_install), the sampler tables (artp_upload_sampler_layers,
 * artp_preprocessed_install, artp_preprocessed_reweight_dev with install_sampler, the roadmap's density rounds) and the
 * motion-cost feature map (artp_cost_update_map, _dev, _layer; artp_cost_load_weights waits for the whole device).  Such a
 * call, issued on the current lane, runs behind everything the other lanes were given before it (they still see the old
 * state), and whatever any lane is given after it runs behind the write (it sees the new state), whether or not the
 * call returns before the device is done.  One thing is left to the caller: a _dev RESULT produced on one lane and passed
 * as an argument to a call on another lane is ordered by the caller (artp_synchronize, or stream events); the library
 * orders its own state, not the caller's buffers.  The current lane is state of the
 * context, not of the calling thread: lanes are for ONE host thread that keeps several batches in flight (threads
 * that share a context would switch each other's lane; give each thread its own context).  No equivalent in the
 * reference (it validates one state at a time on the calling thread). */
int artp_set_lane(artp_ctx* ctx, int lane);
int artp_get_lane(artp_ctx* ctx);

/* ---- map upload: HeightMapBoxChecker::setHeightField
 *      (art_planner/src/validity_checker/height_map_box_checker.cpp:38-54) ----------------------
 * slot 0 = body checker's layer (params.planner.elevation_layer, validity_checker_body.cpp:52-55),
 * slot 1 = feet checker's layer ("elevation_masked", validity_checker_feet.cpp:80-83).
 * Both slots share the grid geometry (also used for grid_map isInside). */
enum { ARTP_SLOT_BODY = 0, ARTP_SLOT_FEET = 1 };
int artp_upload_layer(artp_ctx* ctx, int slot, const float* layer_colmajor, int rows, int cols,
                      double len_x, double len_y, double pos_x, double pos_y);
/* Config-5 incremental update: overwrite the rectangle [row0,row0+nrows) x [col0,col0+ncols) of a
 * previously uploaded layer; `patch` is column-major nrows x ncols. */
int artp_update_layer_rect(artp_ctx* ctx, int slot, const float* patch, int row0, int col0,
                           int nrows, int ncols);
/* Several rectangles of one slot in one call (what computeChange, change.cpp:9-51, yields per map update):
 * patches[k] is column-major nrows x ncols, rects = n_rects x {row0, col0, nrows, ncols}, applied IN ORDER (where
 * rectangles overlap the later one wins).  One staged copy, the range tables rebuilt once, the partner table (kept as
 * counts) re-evaluated for the pairs with an end in a changed rectangle only.  Both forms are ASYNCHRONOUS on the context's stream: the
 * patches are copied to a pinned staging buffer before the call returns (the caller's buffers are free again), the
 * device work is ordered in front of whatever the stream runs next. */
int artp_update_layer_rects(artp_ctx* ctx, int slot, int n_rects, const float* const* patches, const int* rects);
/* Map version of the context: a counter that every call which changes what isValid() / the sampler would answer
 * increments -- artp_upload_layer, artp_update_layer_rect, artp_upload_sampler_layers, artp_preprocessed_install,
 * artp_preprocessed_reweight_dev (when it installs the new distribution).  The reference's guarantee that
 * StateValidityChecker::updateHeightField (validity_checker.cpp:26-29) takes effect for the very next isValid() is
 * what a host-side label cache has to honour: it stamps cached labels with the version they were computed on
 * (artp_sample_and_validate reports it) and compares with artp_map_version() before serving one.  Lock-free read. */
uint64_t artp_map_version(const artp_ctx* ctx);

/* ---- HeightMapBoxChecker::checkCollision (height_map_box_checker.cpp:58-72) -------------------
 * hit[i] = (dCollide(box, field, 1, ...) != 0) for pose i.  exit_codes (optional, may be NULL)
 * receives which early-out of dCollideHeightfieldZone decided (ARTP_EXIT_*). */
enum {
  ARTP_EXIT_AABB_OFF = 0, ARTP_EXIT_ABOVE = 1, ARTP_EXIT_UNDER = 2, ARTP_EXIT_SPANS = 3,
  ARTP_EXIT_FLAT_PLANE = 4, ARTP_EXIT_VERTEX = 5, ARTP_EXIT_PLANE = 6, ARTP_EXIT_VERTEX2 = 7,
  ARTP_EXIT_NONE = 8
};
int artp_check_boxes(artp_ctx* ctx, int slot, const float box_lengths[3], const float* dposes,
                     size_t n, uint8_t* hit, uint8_t* exit_codes);
int artp_check_boxes_dev(artp_ctx* ctx, int slot, const float box_lengths[3], const float* dposes,
                         size_t n, uint8_t* hit, uint8_t* exit_codes);

/* ---- ob::StateValidityChecker::isValid, batched
 *      (art_planner/src/validity_checker/validity_checker.cpp:39-45) ----------------------------
 * valid[i] = body_ok && feet_ok for state i.  detail (optional): n x 6 int8 =
 * {body exit code | -1 outside map, 4 x foot exit code | -1 outside | -2 not evaluated, 0}. */
/* Up to 16 states without `detail` take the latency path: one launch, one workgroup per state with the five
 * boxes side by side, states / labels through mapped pinned host memory (no copies). */
int artp_validate_states(artp_ctx* ctx, const double* se3, size_t n, uint8_t* valid, int8_t* detail);
/* Persistent latency service for the per-state isValid() of the host mirror (validity_checker.cpp:39-45: one OMPL call =
 * one state).  enabled != 0: artp_validate_states calls with one or two states and no `detail` are answered by ONE RESIDENT
 * workgroup that polls a mailbox in mapped host memory -- no kernel launch per call.  The workgroup is started on demand on a
 * stream of its own, restarted after every map write (artp_map_version) and leaves by itself after 200 us without a
 * request (2 s at most in all): it cannot outlive a host that stopped calling, and a burst's end frees the device before
 * a hipFree / hipDeviceSynchronize (which wait for every stream) can trip over it.  Same labels as the launch-per-call path
 * (the same device function).  Off by default: it holds five wavefronts and ~63 KB of LDS of one CU while resident.
 * The same switch covers ob::MotionValidator::checkMotion one edge at a time (prm_motion_cost.cpp:652,
 * lazy_prm_star_min_update.cpp:725, OMPL's PathSimplifier): artp_check_motions / artp_check_motions_last_valid /
 * artp_check_edges_interp calls with one or two edges (host pointers; at most 8 x 256 interpolation states) are answered by a
 * resident POOL of 256 workgroups (one per CU) with the same start / restart / idle rules.  Every workgroup polls a request block in
 * device memory that the host writes through the PCIe BAR, runs its share of the edge's states and reports to a slot of its
 * own in mapped host memory; the host reduces the slots.  (A device that does not expose its memory to the host -- no large
 * BAR -- has no pool: these calls keep their one launch per call.)
 * Same verdicts, lastValid pairs and interpolation counts as the other paths, bit for bit.
 * artp_persistent_latency_stats: out[0] = launches of the resident kernels so far, out[1] = requests they answered. */
int artp_set_persistent_latency(artp_ctx* ctx, int enabled);
int artp_persistent_latency_stats(artp_ctx* ctx, uint64_t out[2]);
int artp_validate_states_dev(artp_ctx* ctx, const double* se3, size_t n, uint8_t* valid,
                             int8_t* detail);

/* ---- ob::StateSampler::sampleUniform, batched
 *      (art_planner/src/sampler.cpp:56-131; SE3FromSE2Sampler) ----------------------------------
 * The seven layers the sampler reads (sampler.cpp:61-63,99-103; map.h:64-116), same geometry as the
 * validity layers.  cum_prob_rowwise = column 0 of "cum_prob_rowwise_hack" (rows floats).
 * A row of cum_prob must be NaN-free or NaN THROUGHOUT.  That is all computeCumulativeProbabilityDistribution can
 * produce (probability_distribution.cpp:28 divides every entry of a row by the row's sum, so a NaN comes from the
 * divisor -- 0 / 0 of an all-zero row, or a NaN cell that poisons the sum -- and then fills the row; the processors
 * only ever multiply finite factors into "sample_probability").  A row that is NaN throughout samples its last column,
 * as the reference's scan does.  For a row that turns NaN part-way the pivot search is undefined: the scan would
 * ignore the NaN entries, the search counts them (tests/test_sampler_probe.py pins the scan's answer). */
int artp_upload_sampler_layers(artp_ctx* ctx, const float* cum_prob, const float* cum_prob_rowwise,
                               const float* elevation, const float* normal_x, const float* normal_y,
                               const float* normal_z, const float* plane_fit_std_dev, int rows,
                               int cols, double len_x, double len_y, double pos_x, double pos_y);
/* State k of the batch is a pure function of (seed, first_index + k): six counter-based uniforms in
 * the reference's draw order replace ompl::RNG's mt19937 stream (SURVEY.md 8c "same seed"). */
int artp_sample_states(artp_ctx* ctx, uint64_t seed, uint64_t first_index, size_t n, double* se3_out);
int artp_sample_states_dev(artp_ctx* ctx, uint64_t seed, uint64_t first_index, size_t n,
                           double* se3_out);
/* Fused rejection-sampling step of the planners' hot loop
 * (prm_motion_cost.cpp:174-186, lazy_prm_star_min_update.cpp:552-554): sample n states, validate
 * them, write states + labels.  n_valid (host pointer, optional) receives the number of valid ones
 * (forces a stream sync when non-NULL). */
int artp_sample_and_validate_dev(artp_ctx* ctx, uint64_t seed, uint64_t first_index, size_t n,
                                 double* se3_out, uint8_t* valid_out, size_t* n_valid);
/* Host-buffer form: states and labels come back together, so a sampler that hands the states out one at a
 * time (ob::StateSampler::sampleUniform) already holds the label the following isValid() will ask for.
 * map_version (optional): the artp_map_version() the states were sampled and validated on (the context's lock is
 * held for the whole call, so it is the version of every label of the batch). */
int artp_sample_and_validate(artp_ctx* ctx, uint64_t seed, uint64_t first_index, size_t n, double* se3_out,
                             uint8_t* valid_out, uint64_t* map_version);

/* ---- Reachability maps: isValid at every cell and heading of a rectangle of the map -----------------
 * The lattice pose of cell (r, c) and heading bin k (0 <= k < n_yaw, 1 <= n_yaw <= 32) is the goal Planner::plan makes
 * of that cell (planner.cpp:224-238, Map::get3DPoseFrom2D, map.cpp:77-90): x, y = the grid_map centre of the cell
 * (the sampler's arithmetic), yaw_k = (2 pi / n_yaw) k, minus 2 pi where it exceeds pi (heading 0 is bin 0), z = the
 * cell's height, roll = -atan2(n_b.y, n_b.z) and pitch = atan2(n_b.x, n_b.z) for the cell's normal turned into the yaw
 * frame, the quaternion from setSO3FromRPY; no perturbation.  Heights and normals are the SAMPLER layers
 * (artp_upload_sampler_layers / artp_preprocessed_install).  Bit k of mask[cell] = the isValid() label of that pose.
 * A cell whose height or any normal component is not finite has mask 0 (its pose is never validated).
 * rect = {row0, col0, nrows, ncols} of the installed map, NULL = the whole map.  mask is column-major nrows x ncols
 * (grid_map's layout; cell (r, c) of the rectangle at r + c nrows).  ARTP_ERR_NO_MAP without both validity layers and
 * the sampler layers; ARTP_ERR_INVALID_ARG for n_yaw outside [1, 32], an empty rect, one not inside the map or
 * nrows * ncols * n_yaw >= 2^32.  The map is validated in chunks of at most 2^22 poses; artp_map_version is unchanged.
 * Host form: synchronous.  _dev form: mask in device memory, asynchronous on the context's current stream / lane. */
int artp_reachability_map(artp_ctx* ctx, int n_yaw, const int rect[4], uint32_t* mask);
int artp_reachability_map_dev(artp_ctx* ctx, int n_yaw, const int rect[4], uint32_t* mask);
/* The lattice poses themselves (x y z qx qy qz qw), host buffer of nrows * ncols * n_yaw states: pose index
 * (r + c nrows) n_yaw + k, so the n_yaw headings of a cell are neighbours.  Cells that are not finite give x, y as above
 * and NaN z and quaternion.  Needs the sampler layers only (ARTP_ERR_NO_MAP otherwise).  Synchronous. */
int artp_reachability_poses(artp_ctx* ctx, int n_yaw, const int rect[4], double* se3_out);
/* *cells = a conservative radius, in cells, of what a cell's mask depends on in the VALIDITY layers: the largest
 * |box offset| + box half-diagonal of the robot (any attitude) over the map resolution, plus the window margin of
 * "diagonal / spacing + 4".  After artp_update_layer_rect(s), which leave the sampler layers alone, recompute the changed
 * rectangle grown by the halo (clipped to the map) and paste it into the old mask: the result equals a full recompute.
 * artp_preprocessed_install (and artp_upload_sampler_layers) change heights and normals too: recompute the whole map. */
int artp_reachability_halo(artp_ctx* ctx, int* cells);

/* ---- Cost-to-go fields: shortest lattice costs from a pose to every cell and heading ------------------
 * The graph: node (r, c, k) of the rectangle at n_yaw headings exists iff bit k of mask[r + c nrows]
 * is set (the layout artp_reachability_map writes; the call never computes the mask: pass an edited or a synthetic one).
 * Ten moves per node: m = 0..7 to the neighbouring cells, (dr, dc) = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1),
 * heading unchanged; m = 8: k -> (k + 1) mod n_yaw; m = 9: k -> (k - 1) mod n_yaw (none at n_yaw = 1).  An edge exists iff
 * both ends exist inside the rectangle and its cost is finite.  Cost of a -> b = PathLengthObjective::motionCost(a, b) on
 * the lattice's nominal numbers: dx = res (-dr), dy = res (-dc) (the difference of the two cell centres), dz = the
 * difference of the sampler layer's cell heights widened to f64, yaw_k as artp_reachability_map defines it.
 *   objective 0: sqrt((dx^2 + dy^2) + dz^2) / max_lon_vel, rotations cost 0
 *   objective 1: max(|lon| / max_lon_vel, |lat| / max_lat_vel, yaw_dif / max_ang_vel), lon = cos(yaw_a) dx + sin(yaw_a) dy,
 *                lat = -sin(yaw_a) dx + cos(yaw_a) dy, yaw_dif = 2 pi / n_yaw for a rotation and 0 for a translation
 *   objective 2 (learned): ARTP_ERR_INVALID_ARG.  The learned objective has its own call, artp_field_compute_learned.
 * dist[node] (f64): reverse = 0: the smallest cost of a lattice path from any source to the node; reverse = 1: from the
 * node to any source.  A path's cost is the left fold ((0 + w1) + w2) + ... of its edge costs counted from the SOURCE end
 * outwards, in both forms.  +inf where the node does not exist or cannot be reached.  The least fixed point of
 * dist[v] = min(dist[u] + w) is unique (fl(+) is monotone, w >= 0), so both kernel forms give the same bits.
 * An edge is usable when both end poses are valid: the interior states of a move are NOT checked.  A lattice path is a
 * proposal; artp_field_path hands its states out as SE3 so that the caller can run them through artp_check_motions, and
 * artp_field_plan (below) does so on the device and takes the verdicts back into the field.
 * Nodes (sources, target, nodes_out) are int triples (r, c, k), r and c LOCAL to the rectangle. */
typedef struct artp_field artp_field;
typedef struct artp_field_params {
  int32_t objective;      /* 0 or 1, as artp_roadmap_params::objective */
  int32_t plain_sweeps;   /* 0 = the tiled form (default); 1 = the plain form: one lane per node, one launch per sweep */
  double max_lon_vel, max_lat_vel, max_ang_vel; /* params.h:71-73; the artp_roadmap_params defaults */
  int32_t inner_sweeps;   /* tiled form: sweeps inside LDS per tile and outer round at most (default 64, >= 1) */
  int32_t reserved;
} artp_field_params;
typedef struct artp_field_stats_t {
  uint64_t outer_rounds;   /* tiled form: kernel launches of the distance search (one host read each) */
  uint64_t tile_launches;  /* tiled form: tiles that ran in them (a launch skips the tiles nothing reached) */
  uint64_t reached_nodes;  /* nodes with a finite distance */
  uint64_t plain_sweeps;   /* plain form: launches of the distance search */
  uint64_t hop_rounds;     /* launches of the hop-count search, either form */
  uint64_t hop_tile_launches;
  uint64_t nodes;          /* nrows * ncols * n_yaw */
  uint64_t tiles;          /* tiles of the rectangle (16 x 16 cells each) */
} artp_field_stats_t;
void artp_field_params_defaults(artp_field_params* p);
/* mask: nrows x ncols words, column-major, in host (mask_on_device = 0) or device memory (1); the field keeps a copy.
 * sources: n_sources >= 1 triples.  Heights are the SAMPLER layers' (ARTP_ERR_NO_MAP without them; the validity layers are
 * not needed).  ARTP_ERR_INVALID_ARG, with nothing computed: n_yaw or rect as artp_reachability_map refuses them, objective
 * not 0 or 1, a velocity that is not positive, a source outside the rectangle or not a node of the mask.  Every launch is
 * bounded; the host reads one count per outer round; more rounds than nodes + 2 (impossible at a fixed point search of
 * non-negative weights) end the call with ARTP_ERR_CAPACITY.  Synchronous, on the context's current stream. */
int artp_field_compute(artp_ctx* ctx, const artp_field_params* params, int n_yaw, const int rect[4], const uint32_t* mask,
                       int mask_on_device, const int* sources, size_t n_sources, int reverse, artp_field** out);
/* dist: nrows * ncols * n_yaw doubles, index (r + c nrows) n_yaw + k (the pose order of artp_reachability_poses).
 * artp_field_dist copies to the host; artp_field_dist_dev gives the field's own device buffer (valid until destroy). */
int artp_field_dist(artp_field* f, double* dist_out);
int artp_field_dist_dev(artp_field* f, const double** dist_dev);
/* Descent from the target along tight predecessors (dist[u] + w == dist[v] bit for bit, one hop closer by the hop count
 * of fewest tight edges, the first such move in the order of the ten moves) to a source.  nodes_out (3 ints per state) and
 * se3_out (7 doubles per state, the poses of artp_reachability_poses; either may be NULL) hold the states in TRAVEL
 * order: source -> target for reverse = 0, target -> source for reverse = 1.  *cost = dist[target].  *n = 0, *cost = +inf
 * and ARTP_OK when the target cannot be reached; ARTP_ERR_CAPACITY with *n = the states needed when cap is too small;
 * ARTP_ERR_INVALID_ARG for a target outside the rectangle. */
int artp_field_path(artp_field* f, const int target[3], int* nodes_out, double* se3_out, size_t cap, size_t* n,
                    double* cost);
/* cost_out[i] = the device's cost of the move a_i -> b_i (host arrays of n triples); NaN where b_i is not one of the ten
 * moves from a_i or a node lies outside the rectangle.  The mask is not consulted. */
int artp_field_edge_costs(artp_field* f, const int* a, const int* b, size_t n, double* cost_out);
int artp_field_stats(artp_field* f, artp_field_stats_t* out);
/* Update the field IN PLACE after its mask (and, on request, its heights) changed in a sub-rectangle (DESIGN.md section
 * 13).  new_mask: nrows x ncols words of the FIELD's rectangle, column-major, host (mask_on_device = 0) or device (1).
 * sub_rect = {row0, col0, nrows, ncols} local to the field's rectangle, NULL = all of it: only the words inside it are
 * read; outside it the field keeps its own words whatever new_mask holds there.  refresh_heights != 0 re-reads the sampler
 * layer's heights inside sub_rect (only objective 0 uses heights).
 * After ARTP_OK dist, hops (artp_field_path), artp_field_edge_costs and reached_nodes are bit for bit those of
 * artp_field_compute with the field's own params, n_yaw, rectangle, sources and reverse on the merged mask and the merged
 * heights (the current ones where refreshed, the old ones elsewhere).  Where the context's map still has the geometry the
 * field was computed on, the poses of artp_field_path are those of the current sampler layers, as a new field's would be.
 * ARTP_ERR_INVALID_ARG with the field untouched: a source is no longer a node of the merged mask, sub_rect is empty or not
 * inside the rectangle, refresh_heights without sampler layers of the geometry the field was computed on, a learned or a
 * clearance-weighted field (artp_field_update_learned and artp_field_update_clearance take those).
 * Every launch is bounded; the round caps are artp_field_compute's.  Synchronous, on the context's current stream. */
typedef struct artp_field_update_stats_t {
  uint64_t changed_words;    /* words of sub_rect that differ in their low n_yaw bits */
  uint64_t removed_nodes;    /* bits cleared */
  uint64_t added_nodes;      /* bits set */
  uint64_t dead_nodes;       /* nodes whose distance lost its support and was recomputed */
  uint64_t hop_dead_nodes;   /* nodes whose hop count lost its support (at the new distances) and was recomputed */
  uint64_t unsupport_rounds; /* launches of the two unsupport passes */
  uint64_t dist_rounds;      /* launches of the distance search */
  uint64_t hop_rounds;       /* launches of the hop-count search */
  uint64_t tile_launches;    /* tiled form: tiles that ran, over all four passes */
  uint64_t reached_nodes;    /* nodes with a finite distance after the update */
} artp_field_update_stats_t;
int artp_field_update(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int sub_rect[4],
                      int refresh_heights);
/* the numbers of the last artp_field_update that returned ARTP_OK (zeros before the first) */
int artp_field_update_stats(artp_field* f, artp_field_update_stats_t* out);
void artp_field_destroy(artp_field* f);

/* ---- Learned-cost fields: cost-to-go under the motion-cost network --------------
 * The same graph, rules and results as artp_field_compute, under the roadmap's objective 2.  The cost of the move a -> b:
 * ONE EdgeMatrix row -- target (x, y, yaw) then start (x, y, yaw) as floats, from the poses artp_reachability_poses gives
 * the two nodes (a lattice move is shorter than any query edge length: no interpolation) -- answered by the network as
 * (energy, time, risk) and priced in f64 as MotionCostObjective prices a chain of one sub-edge:
 *   cost = 0.0 + (energy w_energy + time w_time + risk w_risk), +inf when risk > risk_threshold.
 * An edge whose cost is negative or NaN does not exist (the least fixed point is unique for weights >= 0 only); an edge of
 * cost 0 does.  The cost is NOT symmetric: a -> b and b -> a differ, rotations included, so reverse = 1 is another field.
 * The weights live in a per-field device table of 80 bytes per node (edge tiles padded to 16 x 16 cells), built once per
 * call in chunks of at most 2^22 rows; ARTP_ERR_CAPACITY, with a text, when the device has not that much memory free.
 * The field always prices on the device network, through the kernels artp_cost_query_dev launches (artp_cost_set_fc_path
 * and the load-time self-check hold): a function installed with artp_cost_set_external_query does NOT redirect it, as it
 * does not redirect artp_cost_query.
 * The result is an ordinary artp_field: artp_field_dist, _dist_dev, _path, _edge_costs (the travel-direction cost of
 * a -> b; +inf for an absent edge between neighbouring nodes), _stats and _destroy work on it unchanged.
 * artp_field_update refuses it with ARTP_ERR_INVALID_ARG: a map change moves the network's features, and with them the
 * weights, far beyond any sub-rectangle.  artp_field_update_learned (below) prices the whole table again instead.
 * Statuses, with nothing computed: ARTP_ERR_NO_WEIGHTS without a network, ARTP_ERR_NO_MAP without a feature map
 * (artp_cost_update_map*) or without the sampler layers, ARTP_ERR_INVALID_ARG for a negative or non-finite weight or
 * threshold and for everything artp_field_compute refuses about n_yaw, rect, the sources and inner_sweeps. */
typedef struct artp_field_learned_params {
  float w_energy, w_time, w_risk, risk_threshold; /* the artp_roadmap_params defaults */
  int32_t plain_sweeps, inner_sweeps;             /* as artp_field_params */
} artp_field_learned_params;
typedef struct artp_field_learned_stats_t {
  uint64_t table_rows;   /* slots of the weight table = rows sent through the cost query */
  uint64_t table_bytes;
  uint64_t chunks;       /* query calls */
  double rows_ms, query_ms, combine_ms; /* device time of the three steps of the table build, summed over the chunks */
  double dist_ms, hop_ms;               /* host time of the two searches (every round is read by the host) */
} artp_field_learned_stats_t;
void artp_field_learned_params_defaults(artp_field_learned_params* p);
int artp_field_compute_learned(artp_ctx* ctx, const artp_field_learned_params* params, int n_yaw, const int rect[4],
                               const uint32_t* mask, int mask_on_device, const int* sources, size_t n_sources, int reverse,
                               artp_field** out);
/* the table's six members are zero for a field of artp_field_compute */
int artp_field_learned_stats(artp_field* f, artp_field_learned_stats_t* out);
/* Update a learned field IN PLACE after the cost map, the network or the mask changed.  new_mask and
 * sub_rect as in artp_field_update; new_mask = NULL: the mask did not change (sub_rect is ignored).  The call prices against
 * what the context holds NOW -- the loaded network, the feature map of the last artp_cost_update_map*, the sampler layers --
 * as a new artp_field_compute_learned would; the pricing weights and the threshold stay the field's own.  Every slot of the
 * weight table is priced again (in the chunks of the original build); a slot whose bit pattern changes is written and flags
 * its tile; then the passes of artp_field_update run from the flagged tiles (none when no word and no slot changed).
 * After ARTP_OK dist, hops (artp_field_path), artp_field_edge_costs and reached_nodes are bit for bit those of
 * artp_field_compute_learned with the field's own params, n_yaw, rectangle, sources and reverse on the merged mask and the
 * current context state.  The first update allocates the chunk scratch (36 bytes a row) and keeps it until
 * artp_field_destroy.  artp_field_learned_stats keeps describing the original compute.
 * With the field untouched: ARTP_ERR_INVALID_ARG when the field is not a learned one, sub_rect is empty or not inside the
 * rectangle, a source is no node of the merged mask, or the sampler layers do not have the geometry the field was computed
 * on; ARTP_ERR_NO_WEIGHTS / ARTP_ERR_NO_MAP as artp_field_compute_learned gives them.  A HIP failure (ARTP_ERR_HIP) or
 * ARTP_ERR_CAPACITY after those checks leaves the field UNDEFINED: destroy it.  Synchronous, on the context's stream. */
typedef struct artp_field_learned_update_stats_t {
  uint64_t changed_words, removed_nodes, added_nodes, dead_nodes, hop_dead_nodes, unsupport_rounds, dist_rounds,
      hop_rounds, tile_launches, reached_nodes; /* as artp_field_update_stats_t */
  uint64_t repriced_slots; /* slots of the weight table = rows sent through the cost query */
  uint64_t changed_slots;  /* slots whose weight changed its bit pattern */
  uint64_t weight_tiles;   /* tiles flagged by a changed weight */
  double rows_ms, query_ms, reprice_ms; /* device time of the three steps of the repricing, summed over the chunks */
  double passes_ms;                     /* host time of the four passes (every round is read by the host) */
} artp_field_learned_update_stats_t;
int artp_field_update_learned(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int sub_rect[4]);
/* the numbers of the last artp_field_update_learned that returned ARTP_OK (zeros before the first) */
int artp_field_learned_update_stats(artp_field* f, artp_field_learned_update_stats_t* out);

/* ---- Lazily checked paths on a field: blocked moves, plan, unblock -----------------
 * A field may carry a BLOCKED-MOVE SET: single moves a -> b that are absent edges (weight +inf) although both ends are
 * nodes -- what artp_check_motions says about a move whose interior states fail.  One 16-bit word per node, index as dist;
 * bit j of node v = the edge the field pulls along at v from its neighbour u by offset j (the ten moves' numbering):
 * forward field (reverse = 0): the edge u -> v; reverse field: the edge v -> u.  Only the stated travel direction is
 * blocked: forward and reverse fields of objectives 0 and 1, equal until then, stop being equal once something is blocked.
 * The set is allocated by the first block; a field that never blocked anything behaves and costs as before.
 * After ARTP_OK from any call of this section dist, hops (artp_field_path), artp_field_edge_costs (+inf for a blocked move)
 * and reached_nodes are bit for bit those of a new field on the same mask with the same set blocked in one call.
 * artp_field_update and artp_field_update_learned keep the set: their contract becomes "bit for bit a new field on that
 * state with the same moves blocked".  At n_yaw = 2 moves 8 and 9 are the same rotation: it sits in bits 8 and 9 of its
 * word, which are set, cleared, honoured and counted as ONE move.  A failure of a repair after the checks (ARTP_ERR_HIP,
 * or ARTP_ERR_CAPACITY when a pass exceeds artp_field_compute's cap of nodes + 2 rounds -- not artp_field_plan's
 * cap_states, see there) leaves the field UNDEFINED: destroy it.  Synchronous, on the context's current stream.
 *
 * artp_field_block_moves: a, b = host arrays of n node triples, the moves a_i -> b_i in TRAVEL direction, as
 * artp_field_edge_costs takes them.  *newly_blocked (may be NULL) = moves that were not blocked before.  ARTP_ERR_INVALID_ARG with
 * nothing written: a pair that is not one of the ten moves or has an end outside the rectangle.  Blocking a move whose
 * edge does not exist in the mask sets the bit and changes nothing else. */
int artp_field_block_moves(artp_field* f, const int* a, const int* b, size_t n, uint64_t* newly_blocked);
/* Clears every bit of the nodes whose cell lies in sub_rect ({row0, col0, nrows, ncols} local to the field's rectangle,
 * NULL = all); *unblocked (may be NULL) = moves unblocked.  This is what a caller runs after a map change: a move's verdict
 * depends on the cells its interior states touch, so a sufficient rectangle is the written one grown by
 * artp_reachability_halo() plus one cell.  ARTP_ERR_INVALID_ARG for an empty rectangle or one not inside the field's. */
int artp_field_unblock(artp_field* f, const int sub_rect[4], uint64_t* unblocked);
/* *n = moves blocked; words_out: nrows * ncols * n_yaw words on the host (zeros when nothing was ever blocked) */
int artp_field_blocked_count(artp_field* f, uint64_t* n);
int artp_field_blocked(artp_field* f, uint16_t* words_out);
/* The lazy loop (LazyPRM*'s): for n_targets node triples, paths whose every move passed checkMotion's first overload.
 * Per round, for the targets still pending: the path artp_field_path returns at that moment; all moves of all paths
 * through the batched motion check on the device; the moves that failed blocked; a target whose path held no failing move
 * is finished with that path (later blocks only raise distances and its path stays tight: its cost is the final
 * dist[target]); a target without a path is finished as unreachable; when a bit was newly set the field is repaired once
 * and the others go round again, at most max_rounds (>= 1) rounds a call.
 * statuses[i]: 0 = a checked path, 1 = unreachable (also: not a node of the mask), 2 = rounds exhausted; costs[i] = +inf
 * unless status 0.  path_offsets (n_targets + 1 entries), nodes_out (3 ints a state) and se3_out (7 doubles a state; the
 * states of target i at [path_offsets[i], path_offsets[i + 1]) in travel order as artp_field_path gives them) may be NULL.
 * ARTP_ERR_CAPACITY when cap_states < path_offsets[n_targets]: the output buffers are too small, nothing else.  Statuses,
 * costs and offsets are filled, the field is at its fixed point and artp_field_plan_stats describes the call.
 * The blocks stay on the field after the call, status 2 and that ARTP_ERR_CAPACITY included: a second call continues
 * where the first stopped (after too small a cap_states it finds every path checked and ends in one round).  Refused with nothing changed: what artp_field_path refuses, a changed map (ARTP_ERR_INVALID_ARG: the
 * poses are gone), ARTP_ERR_NO_MAP without both validity layers and artp_set_z_bounds.  The host reads the round's totals
 * once after the descents and the verdicts once after the check, besides the reads of the motion check itself. */
typedef struct artp_field_plan_stats_t {
  uint64_t rounds;                /* descents + checks that ran */
  uint64_t moves_checked;         /* moves sent through checkMotion (a move on two paths counts twice) */
  uint64_t moves_blocked;         /* moves newly blocked */
  uint64_t updates;               /* rounds that repaired the field */
  uint64_t update_tile_runs;      /* tiled form: tiles that ran in those repairs, summed; per round:
                                     artp_field_plan_round_tile_runs */
  uint64_t last_update_tile_runs; /* ... of the last repair alone */
  double descent_ms;              /* stream time of the rounds' descents (field_paths_kernel), summed */
  double check_ms;                /* stream time from there to the end of the block kernel: poses, checkMotion, blocks */
  double round_ms;                /* host time of the same part of the rounds */
  double passes_ms;               /* host time of the repairs (every round of a pass is read by the host) */
} artp_field_plan_stats_t;
int artp_field_plan(artp_field* f, const int* targets, size_t n_targets, int max_rounds, int32_t* statuses, double* costs,
                    uint64_t* path_offsets, int* nodes_out, double* se3_out, size_t cap_states);
/* the numbers of the last artp_field_plan that ran its rounds, whether it returned ARTP_OK or ARTP_ERR_CAPACITY for
 * cap_states (zeros before the first) */
int artp_field_plan_stats(artp_field* f, artp_field_plan_stats_t* out);
/* Per round of that call: the tiles that ran in the round's repair (0 for a round that blocked nothing, and in the plain
 * form).  *n_rounds = the rounds; runs_out (may be NULL with cap = 0) takes the first cap of them. */
int artp_field_plan_round_tile_runs(artp_field* f, uint64_t* runs_out, size_t cap, size_t* n_rounds);

/* ---- Simplified paths: windowed shortcuts, many paths a call --------------------------------
 * What artp_field_plan returns is a lattice staircase, one state per cell or heading step.  This call keeps a subset of
 * each path's states: the cheapest chain of usable shortcuts from the first to the last state, artp_roadmap_simplify_path's
 * search with the candidates limited to a window and everything between the upload of the paths and the read of the
 * result on the device.
 * Path q = the states [offsets[q], offsets[q + 1]) of se3_in (host, 7 doubles a state, travel order, as artp_field_plan
 * hands them out; they need not be lattice poses).  A candidate (i, j) of a path has 1 <= j - i <= window (0 = all pairs).
 * It is usable iff the 0.5 m interpolation rule passes it (artp_check_edges_interp), checkMotion passes it
 * (artp_check_motions) and its cost is finite; its cost is the chain cost of artp_roadmap_simplify_path under the field's
 * objective (0 or 1) and velocities: the sub-edges at the interpolation rule's interior states, summed in order.
 * The search: best[0] = 0; for i ascending, for j ascending, best[j] = best[i] + c(i, j) when that is strictly smaller
 * (the left fold of the sums; the smallest i wins a tie).  With a window of n - 1 or more, or 0, the result is bit for bit
 * artp_roadmap_simplify_path's on a roadmap of the same objective and velocities.  A larger window never costs more.
 * statuses[q]: 0 = simplified; 1 = the input chain itself does not pass: the path comes back unchanged with cost +inf;
 * 2 = an empty path (cost +inf).  costs[q] = best[n - 1] (0 for a single state).  out_offsets (n_paths + 1 entries):
 * path q's kept states at [out_offsets[q], out_offsets[q + 1]) of kept_out (indices into the path, ascending, the first
 * 0 and the last n - 1) and of se3_out (those states); the three may be NULL.  ARTP_ERR_CAPACITY when cap_states <
 * out_offsets[n_paths]: statuses, costs and offsets are filled, nothing else is missing.
 * A clearance-weighted field is accepted and its candidates are priced with the UNWEIGHTED base objective: a shortcut may
 * give back part of the margin the lattice path kept, by at most what a chord over `window` states can cut.
 * Refused with nothing written (ARTP_ERR_INVALID_ARG): a learned field (artp_last_error says so), offsets that do not
 * ascend, a changed map, p == NULL, n_paths == 0 or above 2^24, 2^32 - 1 states or more in one call; ARTP_ERR_NO_MAP
 * without both validity layers and artp_set_z_bounds.
 * Candidates are evaluated in batches of at most max_batch_pairs, cut anywhere; the result does not depend on it.  The
 * host reads the statuses, costs and counts once and the kept indices and states once, besides the reads of the two checks.
 * Synchronous, on the context's current stream; the field itself is not changed. */
typedef struct artp_field_simplify_params {
  uint32_t window;           /* a candidate (i, j) has 1 <= j - i <= window; 0 = all pairs */
  uint32_t reserved;
  uint64_t max_batch_pairs;  /* candidates evaluated per device batch; 0 = the library's default (2^20) */
} artp_field_simplify_params;
typedef struct artp_field_simplify_stats_t {
  uint64_t paths;              /* of the call */
  uint64_t states_in;          /* states of all paths */
  uint64_t states_kept;
  uint64_t candidates;         /* pairs inside the window */
  uint64_t usable_candidates;  /* ... that passed both checks with a finite cost */
  uint64_t batches;
  double eval_ms;              /* stream time of enumeration, the two checks, costs and weights, all batches */
  double search_ms;            /* stream time of the search, the scan of the counts and the output gather */
  double host_ms;              /* host time of the call */
} artp_field_simplify_stats_t;
int artp_field_simplify_paths(artp_field* f, const artp_field_simplify_params* p, const double* se3_in,
                              const uint64_t* offsets, size_t n_paths, int32_t* statuses, double* costs,
                              uint64_t* out_offsets, uint32_t* kept_out, double* se3_out, size_t cap_states);
/* the numbers of the last artp_field_simplify_paths that ran (zeros before the first) */
int artp_field_simplify_stats(artp_field* f, artp_field_simplify_stats_t* out);

/* ---- Clearance maps and clearance-weighted fields -------------------------------------------
 * A cost-to-go field finds the CHEAPEST lattice path, and under PathLengthObjective that path hugs the boundary of the
 * valid set.  A clearance map measures how far every node is from that boundary; a clearance-weighted field prefers to
 * keep away from it.  (The reference declares MinClearanceObjective, objectives/min_clearance_objective.h, but none of its
 * checkers implements clearance(); here the reachability mask is the data.)
 *
 * artp_clearance_map: mask = nrows x ncols words, column-major, the layout of artp_reachability_map; only the low n_yaw
 * bits (1 <= n_yaw <= 32) count, higher bits may hold anything.  OBSTACLE SET of heading k: a cell of the rectangle whose
 * word has ANY of the bits k - yaw_spread .. k + yaw_spread (mod n_yaw) clear (yaw_spread = 0: bit k is clear;
 * yaw_spread = n_yaw / 2: any heading is clear); the cells outside the rectangle are obstacles of every heading iff
 * outside_is_obstacle, and ignored otherwise.  d2[(r + c nrows) n_yaw + k] (uint16, the node order of artp_field_dist):
 *   0        bit k of the node's own word is clear (not a node)
 *   else     the minimum of dr^2 + dc^2 over the obstacles of heading k with dr^2 + dc^2 <= radius_cells^2; offset (0, 0)
 *            counts, so a node can have d2 = 0 when yaw_spread >= 1
 *   0xffff   no such obstacle
 * The value is an exact integer; the clearance in metres is res sqrt(d2).  Needs no installed map, only the context for
 * its stream.  ARTP_ERR_INVALID_ARG, with nothing computed: n_yaw outside [1, 32], radius_cells outside [1, 32],
 * yaw_spread outside [0, n_yaw / 2], outside_is_obstacle not 0 or 1, nrows or ncols < 1, nrows * ncols * n_yaw >= 2^32.
 * Host form (d2_out in host memory): synchronous.  _dev form (d2_dev in device memory): asynchronous on the context's
 * current stream; a host mask (mask_on_device = 0) is copied before either form returns. */
typedef struct artp_clearance_params {
  int32_t radius_cells;        /* R: the cap of the search, 1 .. 32 (default 12) */
  int32_t yaw_spread;          /* s: neighbouring headings that must be valid too, 0 .. n_yaw / 2 (default 0) */
  int32_t outside_is_obstacle; /* 0 (default) or 1 */
  int32_t reserved;
} artp_clearance_params;
void artp_clearance_params_defaults(artp_clearance_params* p);
int artp_clearance_map(artp_ctx* ctx, const artp_clearance_params* params, int n_yaw, int nrows, int ncols,
                       const uint32_t* mask, int mask_on_device, uint16_t* d2_out);
int artp_clearance_map_dev(artp_ctx* ctx, const artp_clearance_params* params, int n_yaw, int nrows, int ncols,
                           const uint32_t* mask, int mask_on_device, uint16_t* d2_dev);
/* artp_field_compute_clearance: the graph, rules and results of artp_field_compute with `base` (objective 0 or 1, heights
 * included), every move priced in f64, in this order of operations, as
 *   w(a -> b) = base(a -> b) (1.0 + gain max(pen(a), pen(b)))
 *   pen(v)    = 0 if d2[v] == 0xffff, else max(0.0, 1.0 - (res sqrt((double)d2[v])) / margin)
 * with d2 = the clearance map of the field's own mask under `clearance` and res = the resolution of the installed map.
 * gain = 0 makes the factor exactly 1.0: the field then equals artp_field_compute's bit for bit.  The weights live in the
 * per-field table of the learned field (80 bytes per node, edge tiles padded; ARTP_ERR_CAPACITY, with a text, when the
 * device has not that much memory free) and the field is searched by the same kernels; it also keeps d2 (2 bytes per node).
 * The result is an ordinary artp_field: artp_field_dist, _dist_dev, _path, _edge_costs, _stats, _block_moves, _unblock,
 * _blocked*, _plan and _destroy work on it unchanged.  artp_field_learned_stats reports its table (table_rows, table_bytes),
 * rows_ms = the device time of the clearance map, combine_ms = that of the table build, chunks = 0, query_ms = 0.
 * A mask edit moves clearances, and with them weights, up to radius_cells around it: artp_field_update and
 * artp_field_update_learned refuse the field with ARTP_ERR_INVALID_ARG and leave it untouched; artp_field_update_clearance
 * (below) updates it in place.
 * ARTP_ERR_INVALID_ARG, with nothing computed: what artp_clearance_map refuses about n_yaw, radius_cells, yaw_spread and
 * outside_is_obstacle; margin not positive or not finite; margin > radius_cells res (clearance beyond the cap is unknown);
 * gain negative or not finite; everything artp_field_compute refuses.  ARTP_ERR_NO_MAP as artp_field_compute. */
typedef struct artp_field_clearance_params {
  artp_field_params base;          /* artp_field_params_defaults */
  artp_clearance_params clearance; /* artp_clearance_params_defaults */
  double margin;                   /* metres: the penalty falls from 1 at an obstacle to 0 at this clearance (default 0.2) */
  double gain;                     /* the factor at an obstacle is 1 + gain (default 2.0) */
} artp_field_clearance_params;
void artp_field_clearance_params_defaults(artp_field_clearance_params* p);
int artp_field_compute_clearance(artp_ctx* ctx, const artp_field_clearance_params* params, int n_yaw, const int rect[4],
                                 const uint32_t* mask, int mask_on_device, const int* sources, size_t n_sources, int reverse,
                                 artp_field** out);
/* the field's own d2 (nrows * ncols * n_yaw words on the host, index as dist); ARTP_ERR_INVALID_ARG for any other field */
int artp_field_clearance(artp_field* f, uint16_t* d2_out);
/* Update a clearance-weighted field IN PLACE after its mask (and, on request, its heights) changed in a sub-rectangle
 * (DESIGN.md section 18).  new_mask, mask_on_device, sub_rect and refresh_heights as in artp_field_update: new_mask covers the
 * field's whole rectangle, only the words inside sub_rect are read (NULL = all), refresh_heights != 0 re-reads the sampler
 * layer's heights inside sub_rect (only base objective 0 uses heights).
 * After the diff of artp_field_update, d2 is computed again on the 16 x 16 tiles that intersect sub_rect grown by
 * radius_cells (a mask word moves no clearance further away), the weight table is priced again on the tiles that intersect
 * sub_rect grown by radius_cells + 1 (a slot depends on its node and one neighbour); a slot whose bit pattern changes is
 * written and flags its tile; then the passes of artp_field_update run from the flagged tiles.  When no word and no height
 * changed the call ends after the diff.  sub_rect = NULL recomputes the clearance map and the table of the whole rectangle.
 * After ARTP_OK dist, hops (artp_field_path), artp_field_clearance, artp_field_edge_costs (every slot of the table) and
 * reached_nodes are bit for bit those of artp_field_compute_clearance with the field's own params, n_yaw, rectangle,
 * sources and reverse on the merged mask and the merged heights, with the same moves blocked.  The poses of
 * artp_field_path follow the current sampler layers as after artp_field_update.  The first update allocates its scratch and
 * keeps it until artp_field_destroy.  artp_field_learned_stats keeps describing the original compute.
 * ARTP_ERR_INVALID_ARG with the field untouched: the field is not a clearance-weighted one, sub_rect is empty or not inside
 * the rectangle, refresh_heights without sampler layers of the geometry the field was computed on, a source is no longer a
 * node of the merged mask.  A HIP failure (ARTP_ERR_HIP) or ARTP_ERR_CAPACITY after those checks leaves the field
 * UNDEFINED: destroy it.  Synchronous, on the context's current stream. */
typedef struct artp_field_clearance_update_stats_t {
  uint64_t changed_words, removed_nodes, added_nodes, dead_nodes, hop_dead_nodes, unsupport_rounds, dist_rounds,
      hop_rounds, tile_launches, reached_nodes; /* as artp_field_update_stats_t */
  uint64_t clearance_tiles; /* tiles whose d2 was computed again */
  uint64_t changed_d2;      /* nodes whose d2 changed */
  uint64_t repriced_slots;  /* slots of the weight table priced again (2560 n_yaw a tile) */
  uint64_t changed_slots;   /* slots whose weight changed its bit pattern */
  uint64_t weight_tiles;    /* tiles flagged by a changed weight */
  double clearance_ms, reprice_ms; /* device time of the two windows */
  double passes_ms;                /* host time of the four passes (every round is read by the host) */
} artp_field_clearance_update_stats_t;
int artp_field_update_clearance(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int sub_rect[4],
                                int refresh_heights);
/* the numbers of the last artp_field_update_clearance that returned ARTP_OK (zeros before the first; after a call that found
 * no change: zeros apart from reached_nodes) */
int artp_field_clearance_update_stats(artp_field* f, artp_field_clearance_update_stats_t* out);

/* ---- A field carried across a map move ---------------------------------------------------
 * A robot-centric map moves with the robot by whole cells.  The context's installed sampler layers are the NEW map; the
 * field still holds the geometry it was computed on.  With si = lround((pos_x_new - pos_x_old) / res) and sj likewise
 * from pos_y -- artp_preprocessed_change's convention: cell (i, j) of the new map lies over cell (i - si, j - sj) of the
 * old one -- node (r, c, k) of the field's rectangle becomes node (r + si, c + sj, k).  The rectangle keeps its map
 * indices {row0, col0, nrows, ncols}: it moves with the map.  new_mask: nrows x ncols words of the rectangle ON THE NEW
 * MAP, the layout artp_reachability_map writes, host (mask_on_device = 0) or device (1); every word is read (after a
 * move a real map's validity changes within the reachability halo of all four borders, not only in the entered strips).
 * After ARTP_OK dist, hops (artp_field_path), artp_field_edge_costs and reached_nodes are bit for bit those of
 * artp_field_compute on the new map with new_mask, the field's own params, n_yaw, rectangle and reverse, its sources
 * moved by (si, sj) and the blocked moves it kept.  Heights (objective 0) move with their cells; the cells that entered
 * take the current sampler layer's; refresh_heights != 0 re-reads the whole rectangle.  The field adopts the context's
 * sampler layers, map version and geometry: artp_field_path's poses, artp_field_plan and artp_field_simplify_paths work
 * as on a new field.  Blocked moves move with their nodes; a slot is cleared when its node left or its neighbour now lies
 * outside the rectangle (artp_field_blocked and _blocked_count report what was kept).  si = sj = 0 is artp_field_update
 * with sub_rect = NULL: the same result and the same counts.
 * Refused with NOTHING written (dist, hops, mask, heights, blocked moves, geometry, sources and all stats stay):
 * ARTP_ERR_INVALID_ARG, with a text in artp_last_error, when the context's map differs from the field's in rows, cols,
 * lengths or resolution, for a learned or a clearance-weighted field (their per-field tables would have to move too:
 * compute a learned field anew, artp_field_shift_clearance below takes the other), when a moved source lies outside the rectangle (no overlap at all included) or is not a node of
 * new_mask, when f or new_mask is NULL; ARTP_ERR_NO_MAP without sampler layers.  A failure after those checks
 * (ARTP_ERR_HIP, ARTP_ERR_CAPACITY) leaves the field UNDEFINED: destroy it.  The first shift allocates its scratch (12
 * bytes a node, 8 a cell) and keeps it.  Synchronous, on the context's current stream. */
typedef struct artp_field_shift_stats_t {
  uint64_t changed_words, removed_nodes, added_nodes, dead_nodes, hop_dead_nodes, unsupport_rounds, dist_rounds,
      hop_rounds, tile_launches, reached_nodes; /* as artp_field_update_stats_t; the first three count the diff between
                                                   the moved mask (0 in the cells that entered) and new_mask */
  int64_t shift_rows, shift_cols; /* si, sj: what the caller adds to its own node coordinates */
  uint64_t kept_cells;            /* cells of the overlap */
  uint64_t left_nodes;            /* nodes of the cells that left the rectangle */
  uint64_t dropped_blocked;       /* blocked moves cleared by the move */
  double move_ms;                 /* stream time of the move */
  double passes_ms;               /* host time of the four passes */
} artp_field_shift_stats_t;
int artp_field_shift(artp_field* f, const uint32_t* new_mask, int mask_on_device, int refresh_heights);
/* the numbers of the last artp_field_shift that returned ARTP_OK (zeros before the first) */
int artp_field_shift_stats(artp_field* f, artp_field_shift_stats_t* out);

/* ---- A clearance-weighted field carried across a map move ---------------------------------
 * artp_field_shift for a field of artp_field_compute_clearance.  Everything said above holds: the shift convention (si, sj),
 * new_mask, the heights and refresh_heights, the blocked moves, and the adoption of the context's sampler layers, map
 * version and geometry.  Behind the move and the diff against new_mask, d2 is computed again over the whole rectangle (after
 * a move the mask changes all round the border), and every slot of the weight table is priced on the new state into a
 * SECOND table, against the weight its own node carried for the same move before the move (+inf where that node's old cell
 * lay outside the rectangle: an entered cell had no edge).  A slot whose bit pattern differs flags its tile, and the passes
 * of artp_field_update run from the flagged tiles.
 * After ARTP_OK dist, hops (artp_field_path), artp_field_clearance, artp_field_edge_costs (every slot) and reached_nodes are
 * bit for bit those of artp_field_compute_clearance on the new map with new_mask, the field's own params, n_yaw, rectangle
 * and reverse, its sources moved by (si, sj) and the blocked moves it kept.  artp_field_dist_dev keeps its buffer.
 * si = sj = 0 is artp_field_update_clearance with sub_rect = NULL: the same result and the same shared counts, and no new
 * allocation.  The first call that moves allocates the second table (80 n_yaw bytes a cell of the padded rectangle, as
 * large as the first) next to the scratch of artp_field_shift, and keeps both until artp_field_destroy; the two tables
 * change roles with every move.
 * Refused with NOTHING written: ARTP_ERR_INVALID_ARG, with a text in artp_last_error, for a field that is not
 * clearance-weighted, and for everything artp_field_shift refuses, for the same reasons (another map size, lengths or
 * resolution; a moved source outside the rectangle or not a node of new_mask; f or new_mask NULL); ARTP_ERR_NO_MAP without
 * sampler layers.  A failure after those checks leaves the field UNDEFINED: destroy it.  Synchronous, on the context's
 * current stream. */
typedef struct artp_field_clearance_shift_stats_t {
  uint64_t changed_words, removed_nodes, added_nodes, dead_nodes, hop_dead_nodes, unsupport_rounds, dist_rounds,
      hop_rounds, tile_launches, reached_nodes; /* as artp_field_shift_stats_t */
  int64_t shift_rows, shift_cols;
  uint64_t kept_cells, left_nodes, dropped_blocked; /* as artp_field_shift_stats_t */
  uint64_t changed_slots; /* slots of the new table whose bit pattern differs from the slot of the same node (the slot's own
                             node: the move's target in a forward field, its origin in a reverse one) and move before the
                             move; a slot whose old cell lay outside the rectangle had +inf */
  uint64_t weight_tiles;  /* tiles flagged by such a slot */
  double move_ms;         /* stream time of the move */
  double clearance_ms;    /* stream time of d2 over the whole rectangle */
  double table_ms;        /* stream time of the table kernel */
  double passes_ms;       /* host time of the four passes */
} artp_field_clearance_shift_stats_t;
int artp_field_shift_clearance(artp_field* f, const uint32_t* new_mask, int mask_on_device, int refresh_heights);
/* the numbers of the last artp_field_shift_clearance that returned ARTP_OK (zeros before the first) */
int artp_field_clearance_shift_stats(artp_field* f, artp_field_clearance_shift_stats_t* out);

/* ---- Many fields in one batched search; pose-to-pose cost matrices -------------
 * artp_field_compute_many: n_sets fields over ONE mask, rectangle, params and direction, one per source set, searched
 * side by side: every round is one launch over (tiles, fields) and one host read of all the fields' counters.  sources
 * holds the triples of all sets one after the other; set b is triples set_offsets[b] .. set_offsets[b + 1] - 1
 * (set_offsets: n_sets + 1 entries, set_offsets[0] = 0, strictly increasing).  out_fields receives n_sets ordinary fields:
 * field b is bit for bit -- dist, hop counts (so paths), edge costs, reached_nodes -- what artp_field_compute gives for
 * set b alone.  Each owns its own copies of the mask, the heights, the table and the flags: artp_field_update, _shift,
 * _block_moves, _plan, _simplify_paths, _path and _destroy work on each one alone, and each is destroyed by the caller.
 * artp_field_stats of field b: outer_rounds / hop_rounds = the rounds of the batch until that field went quiet,
 * tile_launches / hop_tile_launches = its own tile runs, reached_nodes its own.
 * ARTP_ERR_INVALID_ARG, with a text in artp_last_error, every out_fields[b] = NULL and nothing left allocated: everything
 * artp_field_compute refuses (objective 2 included: learned and clearance-weighted fields have no batched form); n_sets
 * of 0 or above 65535; an empty set; offsets that do not increase; plain_sweeps != 0 (the batch runs in the tiled form
 * only); a source that is no node of the mask (the text names the index of its set), before any search runs.
 * ARTP_ERR_CAPACITY, with a text, when hipMemGetInfo shows less free memory than the n_sets fields need (12 bytes per
 * node and cell-sized arrays each).  The round cap is artp_field_compute's.  Synchronous, on the current lane's stream;
 * the call writes no state of the context.
 * artp_field_cost_matrix: matrix_out[i n + j] (n * n doubles on the host) = the cost from pose i to pose j (n triples
 * (r, c, k)), i.e. dist of the forward field of pose i read at pose j: +inf where j cannot be reached from i, 0 on the
 * diagonal, bit for bit artp_field_compute's value.  Not symmetric bit for bit: the two folds run from opposite ends.
 * The fields are computed in groups of at most `batch` (0: the largest group that fits in half of the free device
 * memory), each group's n values per field gathered on the device and read back in one copy, its fields freed before
 * the next group starts.  Both passes run (distances and hop counts).  Refusals as above (a pose that is no node of the
 * mask: the text names the pose), and n of 0 or above 65536.  stats_out may be NULL. */
typedef struct artp_field_many_stats_t {
  uint64_t groups;        /* batched searches */
  uint64_t fields;        /* fields computed: n */
  uint64_t dist_rounds;   /* launches of the distance search, summed over the groups */
  uint64_t hop_rounds;    /* launches of the hop-count search, summed over the groups */
  uint64_t tile_runs;     /* tiles that ran in the distance searches, all fields */
  uint64_t hop_tile_runs; /* tiles that ran in the hop-count searches, all fields */
} artp_field_many_stats_t;
int artp_field_compute_many(artp_ctx* ctx, const artp_field_params* params, int n_yaw, const int rect[4],
                            const uint32_t* mask, int mask_on_device, const int* sources, const uint64_t* set_offsets,
                            size_t n_sets, int reverse, artp_field** out_fields);
int artp_field_cost_matrix(artp_ctx* ctx, const artp_field_params* params, int n_yaw, const int rect[4],
                           const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch,
                           double* matrix_out, artp_field_many_stats_t* stats_out);

/* ---- Batched learned and clearance-weighted fields on one weight table ------------------------
 * The two calls above for the fields of artp_field_compute_learned and artp_field_compute_clearance, whose pull weights
 * sit in a table of 80 bytes per node that does not depend on the sources.  The table is priced ONCE per call, by the
 * single field's own build (learned: rows -> the context's device network -> combine, in its chunks, whatever
 * artp_cost_set_external_query installed; clearance: the clearance map of the mask, then the table kernel), and every
 * field of the batch searches that one table side by side.
 * artp_field_compute_many_*: field b is bit for bit -- dist, hop counts (so paths), edge costs, reached_nodes,
 * artp_field_clearance -- what artp_field_compute_learned / _clearance gives for set b alone on the same context state.
 * Every returned field owns its own copy of the table (a clearance field also of its clearance map and base table),
 * copied device to device in front of the search: artp_field_update_learned, _update_clearance, _shift_clearance,
 * _block_moves, _plan, _path, _edge_costs, _clearance and _destroy work on each one alone.  artp_field_learned_stats of
 * every field describes the shared build (table_rows, table_bytes, chunks and the three build times, the same numbers
 * in every field) and the batch's dist_ms / hop_ms: the host's time for the two batched passes as a whole, not a field's
 * share of them (inside a matrix, each group's own two passes).  artp_field_stats as for artp_field_compute_many.
 * artp_field_cost_matrix_*: matrix_out[i n + j] = that forward field of pose i read at pose j.  Under the learned cost
 * w(a -> b) != w(b -> a): the matrix is not symmetric.  The call owns the one table for all its groups and frees it
 * before it returns; `batch` = 0 sizes the groups by half of the memory that is free once the table stands.
 * table_out (may be NULL): table_builds = 1 however many groups ran, table_copies = 0 (no field of a matrix outlives
 * the call, so none gets a copy), table_rows / table_bytes of the one table, build_ms its stream time.
 * Refused with nothing left allocated, every out_fields[b] = NULL and both stats structs zeroed: everything the single
 * entry point refuses (ARTP_ERR_NO_WEIGHTS, ARTP_ERR_NO_MAP included), everything artp_field_compute_many refuses about
 * sets, offsets and plain_sweeps, a source that is no node of the mask (the text names its set; a matrix checks every
 * pose before it prices anything and names the pose).  ARTP_ERR_CAPACITY, with a text, when hipMemGetInfo shows less free
 * memory than the table, its copies (compute_many only), the build's scratch and the fields need.  Synchronous, on the
 * current lane's stream; no context state is written beyond what artp_field_compute_learned writes. */
typedef struct artp_field_many_table_stats_t {
  uint64_t table_builds;  /* times the weight table was priced: 1 */
  uint64_t table_rows;    /* slots of one table */
  uint64_t table_bytes;   /* bytes of one table */
  uint64_t table_copies;  /* device-to-device copies made for fields that outlive the call */
  double build_ms;        /* stream time of the build */
} artp_field_many_table_stats_t;
int artp_field_compute_many_learned(artp_ctx* ctx, const artp_field_learned_params* params, int n_yaw, const int rect[4],
                                    const uint32_t* mask, int mask_on_device, const int* sources,
                                    const uint64_t* set_offsets, size_t n_sets, int reverse, artp_field** out_fields);
int artp_field_compute_many_clearance(artp_ctx* ctx, const artp_field_clearance_params* params, int n_yaw, const int rect[4],
                                      const uint32_t* mask, int mask_on_device, const int* sources,
                                      const uint64_t* set_offsets, size_t n_sets, int reverse, artp_field** out_fields);
int artp_field_cost_matrix_learned(artp_ctx* ctx, const artp_field_learned_params* params, int n_yaw, const int rect[4],
                                   const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch,
                                   double* matrix_out, artp_field_many_stats_t* stats_out,
                                   artp_field_many_table_stats_t* table_out);
int artp_field_cost_matrix_clearance(artp_ctx* ctx, const artp_field_clearance_params* params, int n_yaw, const int rect[4],
                                     const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch,
                                     double* matrix_out, artp_field_many_stats_t* stats_out,
                                     artp_field_many_table_stats_t* table_out);

/* ---- ob::MotionValidator::checkMotion (OMPL DiscreteMotionValidator; call sites
 *      prm_motion_cost.cpp:652, lazy_prm_star_min_update.cpp:725), batched -----------------------
 * valid[i] = isValid(s2_i) && all interior states of the discretised segment are valid.
 * R^3 bounds for validSegmentCount follow planner.cpp:146-156; z bounds come from
 * artp_set_z_bounds (min/max finite elevation -/+ reach.z/2). */
int artp_set_z_bounds(artp_ctx* ctx, double z_low, double z_high);
/* checkMotion's R^3 maxExtent (the diagonal of the state space's x / y / z bounds; the segment length is 1 % of it)
 * fixed to max_extent instead of following the installed map and the z bounds; 0 = follow them (default).  For hosts that
 * want OMPL's own behaviour: Planner::setMap calls space_->setBounds (planner.cpp:146-163) but nothing re-runs
 * StateSpace::setup(), so longestValidSegment_ stays at the FIRST planned map's extents. */
int artp_set_r3_extent(artp_ctx* ctx, double max_extent);
int artp_check_motions(artp_ctx* ctx, const double* s1, const double* s2, size_t n, uint8_t* valid);
/* Latency form.  The reference calls checkMotion ONE edge at a time on the solution path (prm_motion_cost.cpp:652,
 * lazy_prm_star_min_update.cpp:725, OMPL's PathSimplifier via planner.cpp:272): the HOST-buffer entry points
 * (artp_check_motions, artp_check_motions_last_valid, artp_check_edges_interp) take n <= 64 edges in ONE kernel launch
 * -- edges and verdicts through mapped host memory, no copies, no host round trip for the segment counts.  Same
 * verdicts, lastValid pairs and error codes as the batch pipeline (tests/test_gpu_parity.py).  enabled = 0 sends small
 * calls through the batch pipeline like large ones (default 1). */
int artp_set_few_edges(artp_ctx* ctx, int enabled);
/* How large batches of artp_check_motions run (first overload): two_pass != 0 (default) = s2 and every coarse_stride-th
 * interior state of every edge first, the rest only for the edges still alive (an edge is valid iff all its states are, so
 * the verdicts do not depend on it); two_pass == 0 = one pass over all states.  coarse_stride >= 2, 0 = the default (8). */
int artp_set_edge_passes(artp_ctx* ctx, int two_pass, int coarse_stride);
/* The tail of the batch validity step: what runs behind the two stream passes for the boxes they leave over.  The full
 * tail is five launches that get through any number of such boxes (millions on a map with unknown regions); the rare tail
 * is one launch, a wavefront per box, for the few dozen that terrain without unknown cells leaves.  Both give the same
 * labels for any batch.  mode 0 (default) = pick per call from the count that the previous call OF THE SAME KIND on
 * the lane left behind -- state batches, the first (or only) pass of an edge batch and its second pass keep a count each,
 * since a checkMotion batch alternates two passes of very different size --, and take the full tail on the first such call
 * on a lane and after every map, layer or table write; 1 = always the full tail; 2 = always the
 * rare tail (correct, slow with many leftover boxes).  For tests and A/B runs.  artp_last_tail: the tail the last validity
 * pass queued on the current lane took (1 full, 2 rare, 0 = none yet). */
int artp_set_tail_mode(artp_ctx* ctx, int mode);
int artp_last_tail(artp_ctx* ctx);
int artp_check_motions_dev(artp_ctx* ctx, const double* s1, const double* s2, size_t n,
                           uint8_t* valid);
/* ob::MotionValidator::checkMotion(s1, s2, std::pair<State*, double>& lastValid) (pure virtual in OMPL 1.4.2;
 * DiscreteMotionValidator tests the interior states j = 1 .. nd-1 in order, then s2): for a failing edge
 * last_valid_t[i] = lastValid.second = (j - 1) / nd of the first failing j ((nd - 1) / nd when only s2 fails) and
 * last_valid_se3[i] (n x 7, may be NULL) = interpolate(s1, s2, last_valid_t[i]) = *lastValid.first; a passing
 * edge reports t = 1 and s2 (OMPL leaves lastValid untouched). */
int artp_check_motions_last_valid(artp_ctx* ctx, const double* s1, const double* s2, size_t n, uint8_t* valid,
                                  double* last_valid_t, double* last_valid_se3);
int artp_check_motions_last_valid_dev(artp_ctx* ctx, const double* s1, const double* s2, size_t n, uint8_t* valid,
                                      double* last_valid_t, double* last_valid_se3);
/* PRM-build edge validation of PRMMotionCost::addValidMilestone (prm_motion_cost.cpp:340-377):
 * n_interp = floor(lateral distance / 0.5) interior states at t = step * (1/(n_interp+1)), each
 * must be valid.  n_interp_out optional (uint32 per edge). */
int artp_check_edges_interp(artp_ctx* ctx, const double* s1, const double* s2, size_t n,
                            uint8_t* valid, uint32_t* n_interp_out);
int artp_check_edges_interp_dev(artp_ctx* ctx, const double* s1, const double* s2, size_t n,
                                uint8_t* valid, uint32_t* n_interp_out);

/* ---- batch plumbing around the hot path ---------------------------------------------------------
 * Stream compaction of the valid states (the planners keep only accepted samples,
 * prm_motion_cost.cpp:174-187): out_se3 receives the states with valid[i] != 0 in input order,
 * *n_out_dev (device uint64) their number.  out_se3 must hold n states. */
int artp_compact_valid_dev(artp_ctx* ctx, const double* se3, const uint8_t* valid, size_t n,
                           double* out_se3, uint64_t* n_out_dev);
/* Multi-GPU exchange helpers.  A state is a pure function of (seed, sample index), so ranks exchange the
 * 4-byte indices of their accepted states (RCCL all-gather) and materialise remote states locally:
 * out_idx receives the positions i < n with valid[i] != 0 in order, *n_out_dev their number;
 * artp_sample_states_at_dev writes the states of indices base_index + idx[j], j < min(*count_dev, cap). */
int artp_compact_valid_indices_dev(artp_ctx* ctx, const uint8_t* valid, size_t n, uint32_t* out_idx,
                                   uint64_t* n_out_dev);
int artp_sample_states_at_dev(artp_ctx* ctx, uint64_t seed, uint64_t base_index, const uint32_t* idx,
                              const uint64_t* count_dev, size_t cap, double* se3_out);
/* The most compact form of "which states of my batch were accepted": one bit per candidate (512 KiB for 2^22
 * candidates, against 9 MB of indices or 130 MB of states) -- what the ranks all-gather per batch.
 * bits_out: ceil(n / 64) 64-bit words, bit k of word w = valid[64 w + k] != 0.  artp_indices_from_bits_dev turns
 * the first n bits of a (received) bitmap back into the ascending index list artp_sample_states_at_dev takes. */
int artp_pack_valid_bits_dev(artp_ctx* ctx, const uint8_t* valid, size_t n, uint64_t* bits_out);
/* The receiving side in one call for ALL ranks: bits = n_ranks bitmaps of words_per_rank words each (the all-gather's
 * output), base_index[r] (host array) = first global sample index of rank r's batch.  For every rank the first
 * min(count, cap) accepted states among its first prefix_bits candidates are re-sampled into
 * se3_out[r * cap .. ) (n_ranks x cap x 7 doubles, device); counts_dev[r] (device) = accepted states among the
 * prefix.  Two launches whatever n_ranks is (<= 16). */
int artp_materialise_from_bits_dev(artp_ctx* ctx, uint64_t seed, const uint64_t* bits, int n_ranks,
                                   size_t words_per_rank, size_t prefix_bits, const uint64_t* base_index, size_t cap,
                                   double* se3_out, uint64_t* counts_dev);
int artp_indices_from_bits_dev(artp_ctx* ctx, const uint64_t* bits, size_t n, uint32_t* out_idx, uint64_t* n_out_dev);
/* The second exchange of SURVEY.md 8e: the edge results of a rank as fixed-size records {u32 i, u32 j,
 * f32 cost[3]} (20 bytes; i / j = the caller's vertex ids of the edge's endpoints, cost = the MotionCostFunc row
 * of artp_cost_query_dev or any 3 floats).  records_out (n x 5 u32) receives the records of the edges with
 * valid[e] != 0 in input order, *n_out_dev their number; the block is then all-gathered (RCCL). */
int artp_pack_edge_results_dev(artp_ctx* ctx, const uint8_t* valid, const uint32_t* edge_i, const uint32_t* edge_j,
                               const float* cost, size_t n, uint32_t* records_out, uint64_t* n_out_dev);
/* ---- multi-GPU: device groups --------------------------------------------------------------
 * The path shards over independent sample batches: the map is replicated, rank r of W owns the states
 * [ (step W + r) S, (step W + r + 1) S ) of the (seed, index) sample stream (artp_shard_first_index: gap-free for
 * any W, so labels do not depend on W), and the exchange steps are all-gathers of fixed-size blocks over xGMI.
 * A group owns, for every LOCAL device, one artp_ctx, one RCCL communicator (librccl is bound at run time with
 * dlopen: libartp.so itself does not depend on it), a side stream for the collectives and the double-buffered
 * exchange buffers.  This is what lets a C++ host -- the reference's PlannerRos keeps ONE planner object and calls
 * it from its planning thread, art_planner_ros/src/planner_ros.cpp:250-319 -- use every GPU of the node without an
 * interpreter in the process.  Two ways to build one:
 *   artp_group_create       one process, n devices (ncclCommInitAll); every device gets a host worker thread, so the
 *                           launches of a step are issued in parallel.
 *   artp_group_create_rank  one process per GPU (torchrun / mpirun style): rank 0 makes the id
 *                           (artp_group_unique_id), the launcher distributes its 128 bytes, every rank joins
 *                           (ncclCommInitRank).
 * transport: ARTP_GROUP_RCCL (default) or ARTP_GROUP_PEER_COPY -- single-process groups only: the all-gather as
 * hipMemcpyPeerAsync pushes between the members; it also accepts the SAME device several times, which is how the
 * W > 1 sharding / exchange logic is tested on a one-GPU box.
 * The map: upload / install it on every member's context (artp_group_ctx) -- maps are replicated.  A group call
 * returns the first failing member's status; artp_group_last_error has the text. */
typedef struct artp_group artp_group;
enum { ARTP_GROUP_RCCL = 0, ARTP_GROUP_PEER_COPY = 1 };
#define ARTP_GROUP_ID_BYTES 128
uint64_t artp_shard_first_index(uint64_t step, int rank, int world, uint64_t batch);
int artp_group_create(const int* devices, int n, const artp_params* params, int transport, artp_group** out);
int artp_group_unique_id(uint8_t id[ARTP_GROUP_ID_BYTES]);
int artp_group_create_rank(int device, int rank, int world, const uint8_t id[ARTP_GROUP_ID_BYTES],
                           const artp_params* params, artp_group** out);
void artp_group_destroy(artp_group* g);
const char* artp_group_last_error(const artp_group* g);
int artp_group_world_size(const artp_group* g);
int artp_group_local_count(const artp_group* g);
int artp_group_rank(const artp_group* g, int local);           /* global rank of local member `local` */
artp_ctx* artp_group_ctx(artp_group* g, int local);            /* owned by the group */
/* The number of ranks the transport itself sees: an all-reduce (sum) of ones. */
int artp_group_ranks_seen(artp_group* g, int* ranks_seen);
/* Sizes of the state exchange: batch = S candidates per rank and step; every rank's first
 * min(accepted, materialise_cap) accepted states among its first prefix candidates (0 = all S) are re-materialised
 * on every member after the all-gather (0 = bitmaps only).  (Re)allocates the buffers; drains the group first -- for at
 * most $ARTP_GROUP_CONFIGURE_TIMEOUT_MS milliseconds (default 60000; -1 = wait for ever; a value that is not an integer
 * >= -1 keeps the default), after which the call returns ARTP_ERR_TIMEOUT with nothing reallocated. */
int artp_group_configure(artp_group* g, uint64_t seed, size_t batch, size_t materialise_cap, size_t prefix);
/* One step of the sharded rejection-sampling loop (prm_motion_cost.cpp:174-186 / lazy_prm_star_min_update.cpp:552-554
 * across the node), ASYNCHRONOUS: for every local member -- artp_sample_and_validate_dev on its shard
 * [artp_shard_first_index(step, rank, W, S), + S), one validity bit per candidate (artp_pack_valid_bits_dev), the
 * all-gather of the W bitmaps on the side stream, artp_materialise_from_bits_dev behind it.  Buffers are
 * double-buffered by step parity: step k + 2 waits for step k's exchange on the device, the host never blocks. */
int artp_group_sample_and_validate_step(artp_group* g, uint64_t step);
/* What a step left on member `local` (device pointers, valid once the step's work is done: artp_group_synchronize):
 * se3 / valid = its own S candidates and labels (single-buffered: the next step overwrites them), bits = the W
 * gathered bitmaps (W x ceil(S / 64) words), states = W x materialise_cap x 7 doubles, counts = W accepted counts
 * among the prefix.  Any out pointer may be NULL. */
int artp_group_step_buffers(artp_group* g, int local, uint64_t step, const double** se3, const uint8_t** valid,
                            const uint64_t** bits, const double** states, const uint64_t** counts);
/* The second exchange: per local member the n edges it owns -- valid / edge_i / edge_j / cost as for
 * artp_pack_edge_results_dev (device pointers, on that member's GPU) -- packed into 20-byte records and all-gathered
 * in blocks of `cap` records (n <= cap on every rank; the same cap on every rank).  ASYNCHRONOUS.  Result on every
 * member (artp_group_edge_buffers): records = W x cap x 5 u32, counts = W record counts.  i / j stay in the owner's
 * numbering; add artp_shard_first_index(step, r, W, S) for block r on arrival. */
typedef struct artp_group_edges {
  const uint8_t* valid; const uint32_t* edge_i; const uint32_t* edge_j; const float* cost; size_t n;
} artp_group_edges;
int artp_group_exchange_edges(artp_group* g, const artp_group_edges* per_local, size_t cap);
int artp_group_edge_buffers(artp_group* g, int local, const uint32_t** records, const uint64_t** counts);
/* Waits until every stream of every local member is idle, at most timeout_ms (< 0: no limit).  ARTP_ERR_TIMEOUT
 * names the member and the stream that did not finish (a collective whose peer never arrived) and leaves the group
 * as it is: artp_group_abort tears the communicators down (ncclCommAbort) so that the process can report and exit. */
int artp_group_synchronize(artp_group* g, int timeout_ms);
int artp_group_abort(artp_group* g);

/* Measurement helper: the ALGORITHMIC window size of a batch = sum over states of
 * the heightfield vertices (nMaxX-nMinX+1)*(nMaxZ-nMinZ+1) of all five boxes, no credit for
 * early-outs or short-circuiting, 0 for a box whose centre is outside the map or whose AABB is off
 * the field.  Host result. */
int artp_algorithmic_vertices_dev(artp_ctx* ctx, const double* se3, size_t n, uint64_t* total_vertices);
/* Diagnostics of the last validity batch: out[0] = torso boxes queued for the window stage,
 * out[4] = foot boxes queued, out[1] = boxes that went through the exact plane grouping: queue 2 of the full tail plus
 * the boxes the rare tail (artp_set_tail_mode) grouped itself -- every leftover box that exits and (f) left open, since
 * that tail has no cheaper stage in front of the grouping. */
int artp_debug_pipeline_counters(artp_ctx* ctx, uint64_t out[8]);
/* Diagnostics: the partner table of a layer (one byte per sample in ODE sample layout, bit 0 / bit 1 =
 * the ABC / DBC triangle of the cell has an epsilon-equal plane within *radius cells).
 * out may be NULL to query the radius only; *radius = 0 when the layer has no table. */
int artp_debug_partner_table(artp_ctx* ctx, int slot, uint8_t* out, size_t out_bytes, int* radius);

/* ---- "next" row N1: batched roadmap front end ------------------------------------------
 * Replaces, as one batch per stage, the sampling / connection / search loops of the reference planners:
 *   PRMMotionCostMaintainer::sampleGraph  art_planner/src/planners/prm_motion_cost.cpp:145-219
 *   PRMMotionCost::addValidMilestone      prm_motion_cost.cpp:325-390 (k nearest, 0.5 m interpolation rule)
 *   PRMMotionCost::constructSolution      prm_motion_cost.cpp:536-673 (A*, lazy checkMotion of the path)
 *   PathLengthObjective                   art_planner/src/objectives/path_length_objective.cpp:26-70
 * Vertex 0 = start, vertex 1 = goal, vertices 2.. = the first n_milestones accepted states of the
 * (seed, index) sample stream.  Needs both height layers, the sampler layers and artp_set_z_bounds. */
typedef struct artp_roadmap artp_roadmap;
struct artp_preprocessed;        /* "next" row N2 below */
struct artp_preprocess_params;
typedef struct artp_roadmap_params {
  uint64_t seed, first_index;  /* sample stream */
  uint32_t n_milestones;       /* Params::planner.prm_motion_cost.max_n_vertices (params.h:51) */
  uint32_t k_neighbors;        /* 0 = OMPL KStarStrategy: ceil(e (1 + 1/6) ln n_vertices) */
  int32_t objective;           /* 0 = PathLengthObjective::motionCostHeuristic (Euclidean / max_lon_vel),
                                  1 = directional time cost (use_directional_cost, params.h:70),
                                  2 = learned motion cost: PRMMotionCostMaintainer::updateEdges
                                      (prm_motion_cost.cpp:27-73) over artp_cost_query; needs
                                      artp_cost_load_weights + artp_cost_update_map */
  uint32_t max_replans;        /* bound on lazy edge removals in artp_roadmap_solve */
  double max_lon_vel, max_lat_vel, max_ang_vel; /* params.h:71-73 */
  float w_energy, w_time, w_risk; /* MotionCostObjective::getCost weights (params.h:58-62) */
  float risk_threshold;           /* MotionCostObjective::isFeasible (params.h:55) */
  /* PRMMotionCostMaintainer::sampleGraph's budgets and its in-build re-weighting (prm_motion_cost.cpp:171-193):
   * the graph grows until max_n_vertices (= n_milestones) OR max_n_edges candidate edges OR max_sample_time of
   * sampling; every recompute_density_after_n_samples accepted vertices Map::reApplyPreprocessing() recomputes the
   * sampling distribution from the inverse density of the vertices so far.  0 switches a budget / the re-weighting
   * off.  The re-weighting needs the preprocessing result of the installed map (density_map, artp_preprocess_map_ex)
   * and its parameters; with density_map == NULL the distribution stays fixed. */
  uint32_t max_n_edges;                        /* params.h:52 (default 50000) */
  uint32_t recompute_density_after_n_samples;  /* params.h:53 (default 1000) */
  double max_sample_time;                      /* seconds, params.h:50 (default 2.0) */
  struct artp_preprocessed* density_map;
  const struct artp_preprocess_params* density_params;
  /* How the graph is put together from the accepted-state stream (same stream, same predicates in every mode):
   *   0 = batched (default): all milestones first, k nearest over the FINAL vertex set, symmetrised pairs, one
   *       interpolation-rule verdict and one chain cost per pair.  Fastest; not the reference's graph.
   *   1 = PRMMotionCost::addValidMilestone order (prm_motion_cost.cpp:325-390), the reference's OWN graph: milestones
   *       are inserted one at a time, each is connected to the k = ceil(e (1 + 1/6) ln n) nearest vertices present
   *       at ITS insertion (n = vertices then, itself included; it becomes a neighbour target last), the VALID
   *       PREFIX of every 0.5 m chain stays in the graph as vertices that are neighbour targets for later milestones
   *       (:353-371), start and goal join last (baseSolve, :447-470).  n_milestones is the reference's
   *       max_n_vertices and counts the chain vertices too, max_n_edges counts the sub-edges (:171-172).  The
   *       insertion loop is sequential by construction (host); the interior states of a milestone's k chains are
   *       interpolated and validated as one small device batch.  Vertex ids: 0 start, 1 goal, then insertion order.
   *   2 = LazyPRMStarMinUpdate::addValidMilestone order (lazy_prm_star_min_update.cpp:424-446), BASELINE config 1's
   *       planner: start, goal, then the milestones; vertex i gets DIRECT edges of unknown validity to the
   *       k = ceil(e (1 + 1/6) ln (i + 1)) nearest of its predecessors, validity is established lazily by
   *       artp_roadmap_solve.  Predecessor-only search with a per-vertex k is one batch on the device.
   * In modes 1 and 2 an edge's cost is evaluated ONCE in the direction the reference adds it to its undirected graph
   * (new vertex -> neighbour, along the chain from the milestone: opt_->motionCost(m, n), updateEdges' source ->
   * target) -- visible with the directional and the learned objective; mode 0 evaluates smaller id -> larger id. */
  int32_t construction;
  /* Params::planner.prm_motion_cost.max_query_edge_length (params.h:54, default 0.5): MotionCostObjective::motionCost
   * (motion_cost_objective.cpp:41-42) splits a motion into n_interp = (unsigned)(lateral distance / this) + 1 cost
   * queries -- what prices a path SEGMENT with the learned objective: the shortcut candidates of
   * artp_roadmap_simplify_path and the path costs it compares.  (The GRAPH's sub-edges are priced one query each by
   * PRMMotionCostMaintainer::updateEdges, and the 0.5 m of addValidMilestone's validity chain is a constant of its
   * own, prm_motion_cost.cpp:343: neither depends on this.)  0 = 0.5. */
  double max_query_edge_length;
} artp_roadmap_params;
void artp_roadmap_params_defaults(artp_roadmap_params* p);
/* Samples, connects and validates.  ARTP_ERR_INVALID_ARG (artp_last_error says which) when start or goal
 * is not a valid state (OMPL: INVALID_START / INVALID_GOAL, prm_motion_cost.cpp:452-476). */
int artp_roadmap_build(artp_ctx* ctx, const artp_roadmap_params* params, const double* start_se3,
                       const double* goal_se3, artp_roadmap** out);
/* out[0] vertices, [1] candidate edges, [2] edges passing the interpolation rule, [3] edges removed by
 * the lazy path check so far, [4] k, [5] samples drawn, [6] density re-weightings during the build,
 * [7] bit 0 = the sampling-time budget ended the build, bit 1 = the edge budget cut the vertex set back, bit 2 = the
 * graph is STILL over max_n_edges (the bounded prefix search gave up: treat the budget as not honoured). */
int artp_roadmap_stats(const artp_roadmap* rm, uint64_t out[8]);
/* Any pointer may be NULL.  verts: n_vertices x 7; knn / knn_dist: n_vertices x k (0xffffffff = none);
 * edges_uv: n_edges x 2 (u < v, sorted); edge_*: n_edges. */
int artp_roadmap_export(const artp_roadmap* rm, double* verts, uint32_t* knn, double* knn_dist,
                        uint32_t* edges_uv, uint8_t* edge_valid, uint32_t* edge_interp, double* edge_cost,
                        uint8_t* edge_removed);
/* Cheapest start -> goal path whose edges also pass the discrete motion validator (artp_check_motions).
 * *n_path = 0 when start and goal are not connected; ARTP_ERR_CAPACITY (with *n_path = needed) when
 * path_se3 (cap_states x 7, may be NULL) is too small. */
int artp_roadmap_solve(artp_roadmap* rm, double* path_se3, size_t cap_states, size_t* n_path, double* cost,
                       int* n_replans);
/* LazyPRMStarMinUpdate::baseSolve (lazy_prm_star_min_update.cpp:552-615): the roadmap keeps growing while the
 * planner has time -- solve, then grow by grow_step milestones (artp_roadmap_grow) and solve again until
 * plan_time seconds have passed; the best solution found is returned (the reference keeps bestSolution / bestCost_
 * the same way).  stats (may be NULL): [0] growth rounds, [1] final vertex count, [2] rounds that improved the cost.
 * *n_path = 0 when no round connected start and goal (PlannerStatus::TIMEOUT). */
int artp_roadmap_solve_until(artp_roadmap* rm, double plan_time, uint32_t grow_step, double* path_se3,
                             size_t cap_states, size_t* n_path, double* cost, uint64_t stats[3]);
/* After the map changed (artp_upload_layer / artp_update_layer_rect / artp_preprocessed_install): re-validate
 * every vertex and re-evaluate every edge against the current layers, forget earlier lazy removals -- the
 * batched form of LazyPRMStarMinUpdate's roadmap maintenance (lazy_prm_star_min_update.cpp:18-217).
 * out (may be NULL): [0] vertices now invalid, [1] / [2] edges passing the rule before / after,
 * [3] bit 0 = start still valid, bit 1 = goal still valid. */
int artp_roadmap_revalidate(artp_roadmap* rm, uint64_t out[4]);
/* New start / goal on the kept roadmap: vertices 0 and 1 are replaced and connected to their k nearest
 * vertices (every OMPL query adds its start and goal as milestones, prm_motion_cost.cpp:452-476). */
int artp_roadmap_set_query(artp_roadmap* rm, const double* start_se3, const double* goal_se3);
/* Solution simplification (Params::planner.simplify_solution; the reference calls OMPL's randomised
 * PathSimplifier through ss_->simplifySolution(), planner.cpp:266-280): every pair of path states is tried as a shortcut in one batch
 * (interpolation rule + discrete motion validator + the objective's cost) and the cheapest chain of valid
 * shortcuts is returned -- deterministic, never worse than the input.  out_se3 holds up to n states. */
int artp_roadmap_simplify_path(artp_roadmap* rm, const double* path_se3, size_t n, double* out_se3,
                               size_t* n_out, double* cost);
/* Growing the kept roadmap (PRMMotionCostMaintainer::sampleGraph keeps adding milestones between queries,
 * prm_motion_cost.cpp:145-219; LazyPRM* grows while it plans): the milestones still valid on the CURRENT map
 * stay, n_more new ones are drawn where the sample stream left off, connections (k follows the vertex count)
 * and edge verdicts are recomputed for the whole set.  out (may be NULL) = {milestones kept, milestones the
 * current map invalidated}.  Start and goal must still be valid (else ARTP_ERR_INVALID_ARG: set a new query). */
int artp_roadmap_grow(artp_roadmap* rm, uint64_t n_more, uint64_t out[2]);
/* The preprocessing result re-weightings are computed on (artp_roadmap_params::density_map) belongs to the map it
 * was made from: after a map update hand the roadmap the new one (or NULL) before growing it. */
int artp_roadmap_set_density_map(artp_roadmap* rm, struct artp_preprocessed* pp,
                                 const struct artp_preprocess_params* params);
void artp_roadmap_destroy(artp_roadmap* rm);

/* ---- batched roadmap: one start, many goals ------------------------------------------------------------------------
 * For every goal i the answer of artp_roadmap_set_query(rm, start, goal_i) + artp_roadmap_solve on the same roadmap,
 * from ONE lazy search: the start is attached once, every goal to its own k nearest vertices, and each lazy round is one
 * shortest-path search from the start, one batched motion check of all unresolved paths and the removal of the invalid
 * edges.  Equality with the sequential answers assumes direction-symmetric motion verdicts (DESIGN.md "Many goals from
 * one start").  status[i] / cost[i] (+inf without a path) for every goal; path_offsets (n_goals + 1 entries) and
 * path_se3 (states of goal i at [path_offsets[i], path_offsets[i + 1]), start first, goal last) may be NULL (costs
 * only).  ARTP_ERR_CAPACITY when path_se3 holds fewer than path_offsets[n_goals] states (statuses, costs and offsets are
 * filled).  ARTP_ERR_INVALID_ARG, with nothing changed, when the start is not valid.  The roadmap keeps its query;
 * lazy removals on roadmap edges persist and the motion verdicts are cached, as artp_roadmap_solve does.
 * stats (may be NULL): [0] lazy rounds, [1] edges removed, [2] motions checked, [3] goals answered through the exact
 * set_query + solve fallback (goals that would enter the start's neighbour list or take the start into theirs). */
enum { ARTP_GOAL_SOLVED = 0, ARTP_GOAL_INVALID = 1, ARTP_GOAL_UNREACHABLE = 2, ARTP_GOAL_TOO_MANY_REMOVALS = 3 };
int artp_roadmap_solve_many(artp_roadmap* rm, const double* start_se3, const double* goals_se3, size_t n_goals,
                            int32_t* status, double* cost, uint64_t* path_offsets, double* path_se3,
                            size_t cap_states, uint64_t stats[4]);

/* ---- tree planners: rrt_star, inf_rrt_star, rrt_sharp (art_planner/src/planner.cpp:92-105) ---------------------------
 * OMPL's RRTstar::solve (and InformedRRTstar / RRTsharp) in batch-synchronous form: every batch of `batch` samples is
 * steered, checked, connected and rewired as ONE device batch per stage (DESIGN.md "Tree planners").  The tree's vertex 0
 * is the start; while the goal is not a vertex, slot 0 of each batch is the goal state itself (GoalState's threshold is
 * machine epsilon: it is only reached by steering onto it).  Objectives: PathLengthObjective only (the reference's
 * getObjective, planner.cpp:27-35, never gives the tree planners the learned cost).  Needs both height layers, the
 * sampler layers and artp_set_z_bounds.  The tree is a pure function of the parameters (bit for bit). */
typedef struct artp_tree artp_tree;
typedef struct artp_tree_params {
  uint64_t seed, first_index;  /* sample stream: slot i of batch b is index first_index + b * batch + i */
  int32_t variant;             /* 0 = rrt_star, 1 = inf_rrt_star, 2 = rrt_sharp */
  int32_t objective;           /* 0 = PathLengthObjective::motionCostHeuristic (Euclidean / max_lon_vel),
                                  1 = directional time cost (use_directional_cost, params.h:70); 2 is refused */
  double max_lon_vel, max_lat_vel, max_ang_vel; /* params.h:71-73 */
  uint32_t batch;              /* samples per batch (1 .. 65536; default 1024) */
  uint32_t max_vertices;       /* vertex capacity of the tree (default 100000) */
  uint32_t max_batches;        /* 0 = no limit */
  double plan_time;            /* seconds of artp_tree_grow; 0 = no time budget */
  double range;                /* steering distance; 0 = OMPL's 0.2 x maxExtent (R^3 bounds of planner.cpp:146-156 + pi/2) */
  double rewire_factor;        /* RRTstar's rewireFactor_ (1.1): k = ceil(rewire_factor (e + e/6) ln (n + 1)) <= 64 */
  int32_t profile;             /* != 0: per-stage device times for artp_tree_stage_times (one stream sync per batch) */
} artp_tree_params;
void artp_tree_params_defaults(artp_tree_params* p);
/* ARTP_ERR_INVALID_ARG (artp_last_error says which) when start or goal is not a valid state or a parameter is out of
 * range (objective 2 included).  Creating a tree draws no samples. */
int artp_tree_create(artp_ctx* ctx, const artp_tree_params* params, const double* start_se3, const double* goal_se3,
                     artp_tree** out);
/* Grows by up to n_batches batches (0 = no count limit), stopping early at max_vertices, max_batches or plan_time seconds
 * of this call, whichever comes first (at least one of n_batches, max_batches, plan_time must be set).
 * out (may be NULL): [0] batches run by this call, [1] vertices now. */
int artp_tree_grow(artp_tree* tree, uint64_t n_batches, uint64_t out[2]);
/* The root -> goal chain (n_path states) at cost(goal); *n_path = 0 and *cost = +inf while the goal is not a vertex.
 * Capacity as artp_roadmap_solve: ARTP_ERR_CAPACITY with *n_path = the states needed when cap_states is too small. */
int artp_tree_solve(const artp_tree* tree, double* path_se3, size_t cap_states, size_t* n_path, double* cost);
/* out: [0] vertices, [1] batches, [2] samples drawn, [3] motions checked, [4] rewires, [5] pruned vertices,
 * [6] goal vertex id (~0 = none yet), [7] batch of the first solution (~0 = none yet). */
int artp_tree_stats(const artp_tree* tree, uint64_t out[8]);
/* Any pointer may be NULL.  verts: n x 7; parent (vertex 0: 0xffffffff), cost-to-come, cost of the edge from the parent,
 * batch the vertex was born in, pruned flag: n each.  cost[v] is the left fold from the root of the edge costs along the
 * parent chain: ((0 + w1) + w2) + ... */
int artp_tree_export(const artp_tree* tree, double* verts, uint32_t* parent, double* cost, double* edge_cost,
                     uint32_t* born_batch, uint8_t* pruned);
/* Every motion checkMotion(u, v) checked since creation, in check order: u a vertex, v the vertex id of the new state
 * (0xffffffff when the state did not become one), the verdict, the batch.  *n = the number of motions; the arrays
 * (any may be NULL) take the first cap of them, ARTP_ERR_CAPACITY when they do not hold all. */
int artp_tree_export_checked(const artp_tree* tree, uint32_t* u, uint32_t* v, uint8_t* valid, uint32_t* batch, size_t cap,
                             size_t* n);
/* Planner::getSolutionPath(true): artp_roadmap_simplify_path's all-pairs shortcut search with the tree's objective */
int artp_tree_simplify_path(artp_tree* tree, const double* path_se3, size_t n, double* out_se3, size_t* n_out,
                            double* cost);
/* Device microseconds per stage summed over the batches grown with params.profile != 0: [0] sample, [1] nearest,
 * [2] steer + survivor count, [3] first motion + survivor count, [4] near set, [5] near motions, [6] parent choice,
 * [7] rewire, [8] rrt_sharp shortest paths, [9] cost-to-come (+ pruning). */
int artp_tree_stage_times(const artp_tree* tree, double us[10]);
void artp_tree_destroy(artp_tree* tree);

/* ---- "next" row N2: the per-map preprocessing chain on the device -----------------------
 * Replaces processors::Basic (art_planner/src/map/processors/basic.cpp:42-143: traversability threshold,
 * safety morphology, elevation_masked, sample filter), estimateNormals (art_planner/src/utils.cpp:213-326)
 * and computeCumulativeProbabilityDistribution (processors/probability_distribution.cpp:20-46), which the
 * reference runs on the CPU (OpenCV) on every map update.  Layers are grid_map matrices (float32,
 * column-major rows x cols).  Inpainting (inpaintMatrix, utils.cpp:13-64) stays with the caller: the
 * input layers must be hole-free. */
typedef struct artp_preprocessed artp_preprocessed;
typedef struct artp_preprocess_params {
  float traversability_thres;                    /* Params::planner.traversability_thres (params.h:24) */
  double foothold_margin;                        /* Params::planner.safety.* (params.h:27-34) */
  double foothold_margin_max_hole_size;
  double foothold_margin_max_drop;
  double foothold_margin_max_drop_search_radius;
  double foothold_margin_min_step;
  double foothold_size;
  int use_inverse_vertex_density;                /* Params::sampler.* (params.h:82-84, planner.cpp:43-55) */
  int use_max_prob_unknown_samples;
  double max_prob_unknown_samples;
} artp_preprocess_params;
typedef struct artp_preprocess_inputs { /* column-major rows x cols float layers on the host */
  const float* elevation;       /* required */
  const float* traversability;  /* NULL = all 1 (Basic::checkTraversability, basic.cpp:13-22) */
  const float* observed;        /* NULL = all 1; Basic::addKnownCells (basic.cpp:26-38): cells valid before inpainting */
  const double* vertex_se3;     /* roadmap vertices (n_vertices x 7) for computeInverseSampleDensity; may be NULL */
  size_t n_vertices;
  int rows, cols;
  double len_x, len_y, pos_x, pos_y;
} artp_preprocess_inputs;
void artp_preprocess_params_defaults(artp_preprocess_params* p); /* params.h defaults */
void artp_preprocess_params_yaml(artp_preprocess_params* p);     /* art_planner_ros/config/params.yaml */
/* elevation: required; traversability: NULL = all 1 (Basic::checkTraversability, basic.cpp:13-22).
 * The robot numbers (normal estimation radius, reach) come from the context's artp_params. */
int artp_preprocess_map(artp_ctx* ctx, const float* elevation, const float* traversability, int rows, int cols,
                        double len_x, double len_y, double pos_x, double pos_y,
                        const artp_preprocess_params* params, artp_preprocessed** out);
/* The whole new-map chain of Planner::setUpMapProcessors (planner.cpp:39-58): Basic, then -- when the params ask
 * for it -- computeInverseSampleDensity (sample_density.cpp:12-43: vertices per cell, cv::GaussianBlur of radius
 * (torso.length + torso.width) / 4, probability = max - blurred), applyBaseSampleDistribution,
 * applyMaxUnknownProbability (probability_distribution.cpp:50-90) and the CDF. */
int artp_preprocess_map_ex(artp_ctx* ctx, const artp_preprocess_inputs* in, const artp_preprocess_params* params,
                           artp_preprocessed** out);
/* The old-map chain: computeChange (processors/change.cpp:9-51) between two results of the same size (their
 * origins may differ by whole cells).  updated_out (rows x cols, may be NULL) receives the "updated" layer,
 * rect = {row0, col0, nrows, ncols} bounds the updated cells of the new map (nrows = 0: none). */
int artp_preprocessed_change(artp_ctx* ctx, artp_preprocessed* map_new, const artp_preprocessed* map_old,
                             float height_change_for_update, float* updated_out, int rect[4], uint64_t* n_updated);
/* Hole filling of a layer (rows x cols column-major floats, host): inpaintMatrix (art_planner/src/utils.cpp:13-64,
 * ARTP_INPAINT_PLANNER: NaN cells are the holes, cv::convertTo rounding, column 0 := column 1 / row 0 := row 1
 * afterwards) and the cost node's _elvMapProcess (cost_query_server.py:92-111, ARTP_INPAINT_COST_NODE: non-finite
 * cells are the holes, numpy truncation).  Like the reference the WHOLE layer comes back quantised to 8 bit over
 * [min, max] of its valid cells -- that part is restated exactly; the fill of the hole cells is by default a rim-inwards
 * distance-weighted mean (radius 3, on the device), with ARTP_INPAINT_TELEA Telea's marching like cv::inpaint (host).
 * OpenCV is not available here: both fills are unpinned.  A layer without holes is returned unchanged.
 * *n_holes (optional) = hole cells. */
enum { ARTP_INPAINT_PLANNER = 0, ARTP_INPAINT_COST_NODE = 1,
       /* OR-ed in: fill the holes by Telea's fast-marching method with cv::inpaint's conventions (radius 3; csrc/telea.h:
        * a restatement of the published algorithm, unpinned like everything OpenCV) on the image as the reference hands it
        * to cv::inpaint, instead of the rim-inwards mean.  Host code, ~10 ms for a 400 x 400 layer. */
       ARTP_INPAINT_TELEA = 2 };
int artp_inpaint_layer(artp_ctx* ctx, const float* layer, int rows, int cols, int mode, float* out, uint64_t* n_holes);
/* The fill alone (no context, no GPU): h x w row-major 8-bit image, mask != 0 = pixels to fill, radius `range`
 * (cv::inpaint(img, mask, out, range, cv::INPAINT_TELEA)); out may alias img.  h, w >= 2 (the march reads a 3 x 3
 * neighbourhood; a one-row / one-column layer in artp_inpaint_layer takes the rim-inwards fill instead). */
int artp_telea_inpaint_u8(const uint8_t* img, const uint8_t* mask, int h, int w, int range, uint8_t* out);
/* name: elevation, traversability, normal_x/_y/_z, plane_fit_std_dev, traversability_thresholded_no_safety,
 * traversability_thresholded, elevation_masked, sample_probability, cum_prob, observed, n_samples (the blurred
 * vertex density), traversability_sample_filter, updated (rows x cols floats each) or cum_prob_rowwise (rows). */
int artp_preprocessed_get_layer(artp_ctx* ctx, const artp_preprocessed* pp, const char* name, float* out);
/* Planner::setMap (planner.cpp:135-163): make the result the context's map -- both height fields with
 * their tables, the sampler layers and the z bounds.  When the context already holds a map of the same geometry, each
 * height field is compared with the installed one bit for bit first: an identical layer keeps its tables, a layer that
 * differs inside a rectangle of at most a quarter of the map is rewritten there only and its tables take the
 * rectangle-update path (artp_update_layer_rects) -- the same tables as a fresh install, at the cost of the change. */
int artp_preprocessed_install(artp_ctx* ctx, const artp_preprocessed* pp);
/* Map::reApplyPreprocessing (art_planner/src/map/map.cpp:94-96), the part that can change on an unchanged map:
 * the sampling distribution re-weighted by the inverse density of the given roadmap vertices (DEVICE pointer,
 * n x 7 doubles; NULL / 0 = no density term) and its CDF.  With install_sampler != 0 the context's sampler uses
 * the new CDF from the next sample on (the height fields are untouched). */
int artp_preprocessed_reweight_dev(artp_ctx* ctx, artp_preprocessed* pp, const struct artp_preprocess_params* params,
                                   const double* vertex_se3_dev, size_t n_vertices, int install_sampler);
void artp_preprocessed_destroy(artp_preprocessed* pp);

/* ---- learned motion cost: MotionCostObjective::MotionCostFunc
 *      (art_planner/include/art_planner/objectives/motion_cost_objective.h:22-23; the reference
 *      implements it as a ROS service to the Python/CUDA node, art_planner_ros/src/planner_ros.cpp:
 *      283-318 -> art_planner_motion_cost/scripts/cost_query_server.py:145-169) ----------------------
 * Weights: a flat float32 blob of the network with eval-mode BatchNorm folded into every convolution:
 * "ARMC", a version byte, 3 pad bytes, then for the six convolutions [Cout][Cin][KH][KW] weights + [Cout] bias,
 * then the 1x1 layers tar0, out0, out1_conv1..3 ([Cout][Cin] + [Cout]) and out2_conv1..3 ([Cin] + 1).
 *   version 1: the light n48convNetwork3LR (network_light.py:19-62): conv1/2 24, conv3..5 and the 15x15 layer 48
 *              channels, out0 64 -> 48, heads 24 / 24 / 36; 583 379 floats (2 333 524 bytes).
 *   version 2: the full-width n9convNetwork3LR (network.py: grid-1563-blind, grid-1975-blind, grid-1992-perceptive):
 *              conv1/2 32, then 64 channels, out0 80 -> 64, heads 32 / 32 / 32; 1 035 283 floats (4 141 140 bytes).
 * tools/convert_weights.py writes either from a torch state_dict (init_conv1's width picks the version). */
size_t artp_cost_blob_bytes(void);                 /* the version-1 (light) size */
size_t artp_cost_blob_bytes_version(int version);  /* the size of a version-1 or -2 blob; 0 for any other version */
/* Either version; a context switches networks in either direction.  A load that changes the network drops the
 * feature map: artp_cost_query* answer ARTP_ERR_NO_MAP until the next artp_cost_update_map* (no query is ever answered
 * from the other network's features).  Reloading the same network keeps it, as before. */
int artp_cost_load_weights(artp_ctx* ctx, const void* blob, size_t bytes);
/* *channels = the feature channels of the loaded network: 48 (version 1) or 64 (version 2); ARTP_ERR_NO_WEIGHTS before a load. */
int artp_cost_feature_channels(artp_ctx* ctx, int* channels);
/* Which kernel answers artp_cost_query: *mfma = 1 the MFMA form of FCpart (network_light.py:113-165), 0 the fp32 VALU kernels.
 * artp_cost_load_weights runs a probe batch through both and falls back to fp32 if they disagree (*selfcheck: 1 agreed,
 * 0 disagreed, -1 not run; *max_abs_diff = the probe's largest difference).  Any pointer may be NULL. */
int artp_cost_fc_path(artp_ctx* ctx, int* mfma, int* selfcheck, float* max_abs_diff);
/* mfma == 0: artp_cost_query on the fp32 VALU kernels (comparison / a toolchain whose self-check fails); != 0 (default): the
 * MFMA form, entered only through the self-check.  Before artp_cost_load_weights it sets what the load will choose. */
int artp_cost_set_fc_path(artp_ctx* ctx, int mfma);
/* CostPredictor.updateFeatures (predictor.py:28-36) + CostQuery.setMapParams (cost_query.py:26-35):
 * elev_xy is the server's map array [rows][cols] row-major with index a growing along world x and b
 * along world y (cost_query_server.py:66-74), holes already inpainted; (cx, cy) = map centre.
 * A map smaller than 54 x 54 (a feature map under 3 x 3) is refused with ARTP_ERR_INVALID_ARG; a refused update changes
 * nothing a query sees: the previous map's features and geometry keep answering (as does artp_cost_debug_forms). */
int artp_cost_update_map(artp_ctx* ctx, const float* elev_xy, int rows, int cols, double res, double len_x,
                         double len_y, double cx, double cy);
/* The same with the map array already in HBM (asynchronous on the context's stream). */
int artp_cost_update_map_dev(artp_ctx* ctx, const float* elev_xy_dev, int rows, int cols, double res, double len_x,
                             double len_y, double cx, double cy);
/* The same from the planner's grid_map elevation layer (column-major rows x cols, as PlannerRos publishes it
 * to the cost node): applies the server's rot90(.., 2).transpose() re-indexing (cost_query_server.py:66-74).
 * Holes (NaN / inf) are an error unless artp_cost_set_hole_filling is on (cost_query_server.py:90-111). */
int artp_cost_update_map_layer(artp_ctx* ctx, const float* layer, int rows, int cols, double res, double len_x,
                               double len_y, double pos_x, double pos_y);
/* enabled != 0: artp_cost_update_map_layer fills the holes of its layer itself (artp_inpaint_layer,
 * ARTP_INPAINT_COST_NODE) instead of rejecting it -- the node's behaviour (cost_query_server.py:92-111).
 * enabled == 2: with Telea's fill (ARTP_INPAINT_TELEA), the algorithm the node calls. */
int artp_cost_set_hole_filling(artp_ctx* ctx, int enabled);
/* MotionCostFunc: edges [B][6] = target x y yaw, start x y yaw (prm_motion_cost.cpp:41-52);
 * cost [B][3] = energy, time, risk (= 1 - prob; cost_query.py:65-69). */
int artp_cost_query(artp_ctx* ctx, const float* edges, size_t b, float* cost);
int artp_cost_query_dev(artp_ctx* ctx, const float* edges, size_t b, float* cost);
/* The MotionCostFunc seam of PRMMotionCostMaintainer (prm_motion_cost.cpp:27-73: `func(edge_matrix, &edge_cost)` -- in
 * PlannerRos a ROS service client, planner_ros.cpp:283-318).  With fn != NULL every batch the ROADMAP prices with the
 * learned objective (artp_roadmap_params::objective == 2: build, grow, revalidate, set_query, simplify_path) goes
 * through the caller's function instead of the device network: edges / cost are HOST buffers in artp_cost_query's
 * layout, return 0 on success; any other value fails the roadmap call with ARTP_ERR_COST_FUNC (the reference throws
 * std::runtime_error("Motion cost call failed"), motion_cost_objective.cpp:78-83).  No weights need to be loaded then.
 * fn == NULL (default): device pricing (artp_cost_query_dev).  artp_cost_query itself is never redirected. */
typedef int (*artp_cost_query_fn)(void* user, const float* edges, size_t b, float* cost);
int artp_cost_set_external_query(artp_ctx* ctx, artp_cost_query_fn fn, void* user);
/* diagnostics: the feature-map cell (row, col) CostQuery.__call__ gathers for each edge's start position
 * (cost_query.py:54-55: float64 arithmetic, clamp to [1, shape - 2], .long()) -- computed by the device function the
 * cost kernels use; the tests compare it with the reference's own CostQuery.  Host buffers. */
int artp_cost_debug_query_cells(artp_ctx* ctx, const float* edges, size_t b, int32_t* rows_out, int32_t* cols_out);
/* diagnostics: the kernel forms the last successful artp_cost_update_map* ran: out[0] the network version (1 / 2),
 * out[1] conv345_kernel's tile edge (12 / 16 / 18), out[2] the 15 x 15 layer's tile height in rows (6 / 8 / 9 / 10),
 * out[3] its workgroup size in threads (256 / 512).  All zero before the first successful update. */
int artp_cost_debug_forms(artp_ctx* ctx, int out[4]);
/* diagnostics: feature map as float [fh][fw][48]; out may be NULL to query the size.  The light network's 48 channels
 * only: ARTP_ERR_INVALID_ARG while a version-2 network is loaded (use artp_cost_get_features_c). */
int artp_cost_get_features(artp_ctx* ctx, float* out, int* fh, int* fw);
/* the same for either network: float [fh][fw][channels]; channels must be artp_cost_feature_channels' value
 * (ARTP_ERR_INVALID_ARG otherwise) */
int artp_cost_get_features_c(artp_ctx* ctx, float* out, int channels, int* fh, int* fw);

#ifdef __cplusplus
}
#endif
#endif /* ARTP_C_H */
