// reach.h -- reachability maps: StateValidityChecker::isValid at every cell and heading of a rectangle of the map.
//
// The lattice pose of cell (r, c) and heading bin k is what Planner::plan makes of a goal at that cell centre and yaw
// (planner.cpp:224-238): x, y = the grid_map centre of the cell, yaw_k = 2 pi k / n_yaw wrapped to (-pi, pi], z, roll and
// pitch from Map::get3DPoseFrom2D (map.cpp:77-90: the cell's height, its normal turned into the yaw frame), the
// quaternion from setSO3FromRPY -- the sampler's arithmetic without its perturbation.  Bit k of mask[cell] is the
// pipeline's label of that pose.
//   reach_poses_kernel  one lane per pose (pose index = (r_local + c_local nrows) n_yaw + k: the n_yaw poses of a cell are
//                       neighbours); the poses leave through LDS as coalesced rows, the PoseRecs of the validity pipeline
//                       are made while the pose is in registers
//   reach_pack_kernel   one lane per cell: its n_yaw labels -> one uint32, 0 for a cell whose height or normal is not finite
// Cells whose height or normal is not finite have NaN z and quaternion; the pipeline never sees those numbers: their
// PoseRec is a finite stand-in (the cell centre at z = 0, identity attitude) whose label the pack kernel discards.
#pragma once

namespace artp {

constexpr int ARTP_REACH_MAX_YAW = 32;
constexpr size_t ARTP_REACH_CHUNK = size_t(1) << 22;  // poses per pipeline call (bounds pose_recs and the queues)

struct ReachRect {
  int row0, col0, nrows, ncols;
  int n_yaw;
};

__device__ __forceinline__ bool reach_cell_finite(const float4& ca) {
  return is_finite(ca.x) && is_finite(ca.y) && is_finite(ca.z) && is_finite(ca.w);
}

// The lattice pose (x y z qx qy qz qw) of pose index p of the rectangle; false (NaN z and quaternion) where the cell's
// height or normal is not finite.
__device__ __forceinline__ bool reach_lattice_pose(const SamplerDev& sm, const MapGeom& g, const ReachRect& rc, uint32_t p,
                                                   double* st) {
  const uint32_t cell = p / (uint32_t)rc.n_yaw;
  const int k = (int)(p - cell * (uint32_t)rc.n_yaw);
  const int row = rc.row0 + (int)(cell % (uint32_t)rc.nrows);
  const int col = rc.col0 + (int)(cell / (uint32_t)rc.nrows);
  // grid_map getPosition: (c + (L/2 - res/2)) + res * (-i), as the sampler computes it
  const double px = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) + g.res * (double)(-row);
  const double py = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) + g.res * (double)(-col);
  // the n_yaw lanes of a cell read the same 32-byte record: one request for all of them
  const float4 ca = sm.cells[2 * ((size_t)row + (size_t)col * g.rows)];
  const bool fin = reach_cell_finite(ca);
  const double pi = 3.14159265358979323846;
  double yaw = (2.0 * pi / (double)rc.n_yaw) * (double)k;
  if (yaw > pi) yaw -= 2.0 * pi;
  st[0] = px;
  st[1] = py;
  {
    const double nwx = (double)ca.y, nwy = (double)ca.z, nwz = (double)ca.w;
    double sy2s, sy2c;
    sincos_half_angle(0.5 * yaw, &sy2s, &sy2c);
    // normal_b = Quaterniond(AngleAxisd(yaw, Z)).inverse() * normal_w: the plane rotation by -yaw (as sample_one)
    const double cyaw = sy2c * sy2c - sy2s * sy2s, syaw = (sy2c + sy2c) * sy2s;
    const double nbx = cyaw * nwx + syaw * nwy;
    const double nby = cyaw * nwy - syaw * nwx;
    const double nbz = nwz;
    const double roll = -atan2(nby, nbz);
    const double pitch = atan2(nbx, nbz);
    double cr, cp, sr, sp;  // setSO3FromRPY (utils.h:101-115)
    sincos_half_angle(roll * 0.5, &sr, &cr);
    sincos_half_angle(pitch * 0.5, &sp, &cp);
    const double cy = sy2c, sy = sy2s;
    st[2] = (double)ca.x;
    st[6] = cy * cp * cr + sy * sp * sr;
    st[3] = cy * cp * sr - sy * sp * cr;
    st[4] = sy * cp * sr + cy * sp * cr;
    st[5] = sy * cp * cr - cy * sp * sr;
  }
  if (!fin) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = 2; j < 7; ++j) st[j] = nan;
  }
  return fin;
}

// Poses first_pose .. first_pose + n - 1 of the rectangle; se3_out / recs (either may be null) point at pose first_pose.
__global__ void __launch_bounds__(256)
reach_poses_kernel(SamplerDev sm, MapGeom g, ReachRect rc, uint32_t first_pose, uint32_t n, double* __restrict__ se3_out,
                   FieldDev f, PoseRec* __restrict__ recs) {
  __shared__ double stage[4][64 * 8];  // 64 poses x 7 doubles, then 64 PoseRecs x 64 bytes
  const int lane = threadIdx.x & 63;
  double* sw = stage[threadIdx.x >> 6];
  const uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x - lane);  // wave-uniform
  if (i0 >= n) return;
  const uint32_t i = i0 + lane;
  float4 r[4];
  if (i < n) {
    double st[7];
    const bool fin = reach_lattice_pose(sm, g, rc, first_pose + i, st);
    if (se3_out) {
#pragma unroll
      for (int j = 0; j < 7; ++j) sw[lane * 7 + j] = st[j];
    }
    if (recs) {
      if (!fin) {  // finite stand-in: the label is discarded by reach_pack_kernel
        st[2] = 0.0;
        st[3] = st[4] = st[5] = 0.0;
        st[6] = 1.0;
      }
      make_pose_rec(f, st, r);
    }
  }
  const uint32_t live = n - i0 < 64u ? n - i0 : 64u;
  if (se3_out) {
    wave_lds_sync();
    const uint32_t cnt = live * 7;
    double* out = se3_out + 7 * (size_t)i0;
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if ((uint32_t)(k * 64 + lane) < cnt) __builtin_nontemporal_store(sw[k * 64 + lane], &out[k * 64 + lane]);
  }
  if (recs) {
    wave_lds_sync();
    float4* rw = reinterpret_cast<float4*>(sw);
    if (i < n) stage_pose_rec(rw, lane, r);
    wave_lds_sync();
    flush_pose_recs(rw, lane, live, recs + i0);
  }
}

// Cells first_cell .. first_cell + n_cells - 1 of the rectangle: labels (n_cells x n_yaw bytes, cell-major) -> mask
// (the whole rectangle's column-major nrows x ncols words; this launch writes its cells only).
__global__ void __launch_bounds__(256)
reach_pack_kernel(SamplerDev sm, MapGeom g, ReachRect rc, uint32_t first_cell, uint32_t n_cells,
                  const uint8_t* __restrict__ labels, uint32_t* __restrict__ mask) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cells) return;
  const uint32_t cell = first_cell + j;
  const int row = rc.row0 + (int)(cell % (uint32_t)rc.nrows);
  const int col = rc.col0 + (int)(cell / (uint32_t)rc.nrows);
  const float4 ca = sm.cells[2 * ((size_t)row + (size_t)col * g.rows)];
  uint32_t bits = 0;
  const uint8_t* l = labels + (size_t)j * rc.n_yaw;
  for (int k = 0; k < rc.n_yaw; ++k) bits |= (l[k] ? 1u : 0u) << k;
  mask[cell] = reach_cell_finite(ca) ? bits : 0u;
}

}  // namespace artp

namespace {

// rect (NULL = the whole map) and n_yaw against the installed map; *out = the rectangle
int reach_resolve(artp_ctx* c, int n_yaw, const int* rect, artp::ReachRect* out) {
  if (n_yaw < 1 || n_yaw > artp::ARTP_REACH_MAX_YAW) {
    c->last_error = "n_yaw must lie in [1, 32]";
    return ARTP_ERR_INVALID_ARG;
  }
  const int rows = c->geom.rows, cols = c->geom.cols;
  artp::ReachRect r{0, 0, rows, cols, n_yaw};
  if (rect) r = artp::ReachRect{rect[0], rect[1], rect[2], rect[3], n_yaw};
  if (r.nrows < 1 || r.ncols < 1 || r.row0 < 0 || r.col0 < 0 || r.row0 > rows - r.nrows || r.col0 > cols - r.ncols) {
    c->last_error = "rect is empty or not inside the map";
    return ARTP_ERR_INVALID_ARG;
  }
  if ((uint64_t)r.nrows * (uint64_t)r.ncols * (uint64_t)n_yaw >= (1ull << 32)) {
    c->last_error = "nrows * ncols * n_yaw must stay below 2^32";
    return ARTP_ERR_INVALID_ARG;
  }
  *out = r;
  return ARTP_OK;
}

// the sampler layers hold the heights and normals of the lattice: they must cover the installed grid
bool reach_have_lattice(const artp_ctx* c) {
  return c->have_sampler && c->have_geom && c->sampler_rows == c->geom.rows && c->sampler_cols == c->geom.cols;
}

// cells per pipeline call: whole cells, at most ARTP_REACH_CHUNK poses
size_t reach_chunk_cells(int n_yaw) { return artp::ARTP_REACH_CHUNK / (size_t)n_yaw; }

}  // namespace

extern "C" {

int artp_reachability_map_dev(artp_ctx* c, int n_yaw, const int* rect, uint32_t* mask) {
  if (!c || !mask) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!c->have_field[0] || !c->have_field[1] || !reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  artp::ReachRect r;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, &r));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t cells = (size_t)r.nrows * r.ncols, per = reach_chunk_cells(n_yaw);
  const size_t chunk_poses = (cells < per ? cells : per) * (size_t)n_yaw;
  ARTP_TRY(ensure_recs(c, chunk_poses));
  ARTP_TRY(ensure_scratch(c, c->lane->call_scratch, chunk_poses));  // the chunk's labels
  for (size_t c0 = 0; c0 < cells; c0 += per) {
    const size_t nc = cells - c0 < per ? cells - c0 : per;
    const size_t np = nc * (size_t)n_yaw;
    uint8_t* labels = c->lane->call_scratch.as<uint8_t>();
    hipLaunchKernelGGL(artp::reach_poses_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->lane->stream, c->sampler,
                       c->geom, r, (uint32_t)(c0 * (size_t)n_yaw), (uint32_t)np, (double*)nullptr, c->field[0],
                       c->lane->pose_recs.as<PoseRec>());
    HIP_TRY(c, hipGetLastError());
    ARTP_TRY(launch_validate_pipeline(c, nullptr, np, labels, true));
    hipLaunchKernelGGL(artp::reach_pack_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, c->lane->stream, c->sampler,
                       c->geom, r, (uint32_t)c0, (uint32_t)nc, (const uint8_t*)labels, mask);
    HIP_TRY(c, hipGetLastError());
  }
  return ARTP_OK;
}

int artp_reachability_map(artp_ctx* c, int n_yaw, const int* rect, uint32_t* mask) {
  if (!c || !mask) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!c->have_field[0] || !c->have_field[1] || !reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  artp::ReachRect r;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, &r));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t cells = (size_t)r.nrows * r.ncols;
  ARTP_TRY(ensure_scratch(c, c->lane->host_args, cells * sizeof(uint32_t)));
  ARTP_TRY(artp_reachability_map_dev(c, n_yaw, rect, c->lane->host_args.as<uint32_t>()));
  HIP_TRY(c, hipMemcpyAsync(mask, c->lane->host_args.get(), cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->lane->stream));
  return check_error_flag(c);
}

int artp_reachability_poses(artp_ctx* c, int n_yaw, const int* rect, double* se3_out) {
  if (!c || !se3_out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  artp::ReachRect r;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, &r));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t cells = (size_t)r.nrows * r.ncols, per = reach_chunk_cells(n_yaw);
  const size_t chunk_poses = (cells < per ? cells : per) * (size_t)n_yaw;
  ARTP_TRY(ensure_scratch(c, c->lane->host_args, chunk_poses * 7 * sizeof(double)));
  for (size_t c0 = 0; c0 < cells; c0 += per) {
    const size_t nc = cells - c0 < per ? cells - c0 : per;
    const size_t np = nc * (size_t)n_yaw, first = c0 * (size_t)n_yaw;
    hipLaunchKernelGGL(artp::reach_poses_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->lane->stream, c->sampler,
                       c->geom, r, (uint32_t)first, (uint32_t)np, c->lane->host_args.as<double>(), c->field[0],
                       (PoseRec*)nullptr);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(se3_out + 7 * first, c->lane->host_args.get(), np * 7 * sizeof(double), hipMemcpyDeviceToHost, c->lane->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

int artp_reachability_halo(artp_ctx* c, int* cells) {
  if (!c || !cells) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!c->have_geom || !(c->geom.res > 0.0)) return ARTP_ERR_NO_MAP;
  const artp_params& p = c->params;
  // a box of a lattice pose lies within |offset| + its 3-D half-diagonal of the cell centre, whatever the attitude
  const double tox = p.torso_off_x, toy = p.torso_off_y, toz = p.torso_off_z - p.feet_off_z;
  const double torso = std::sqrt(tox * tox + toy * toy + toz * toz) +
                       0.5 * std::sqrt(p.torso_length * p.torso_length + p.torso_width * p.torso_width +
                                       p.torso_height * p.torso_height);
  const double feet = std::sqrt(p.feet_off_x * p.feet_off_x + p.feet_off_y * p.feet_off_y) +
                      0.5 * std::sqrt(p.reach_x * p.reach_x + p.reach_y * p.reach_y + p.reach_z * p.reach_z);
  const double reach = torso > feet ? torso : feet;
  // the samples a box check reads: its footprint plus the window margin of "diagonal / spacing + 4"
  *cells = (int)std::ceil(reach / c->geom.res) + 4;
  return ARTP_OK;
}

}  // extern "C"
