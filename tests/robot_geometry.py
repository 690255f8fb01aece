"""Robots other than the two presets (TEST INFRASTRUCTURE; tests/test_robot_geometry_ref.py pins on the CPU what these
inputs reach, tests/test_robot_geometry.py runs them on the GPU).

Nearly every kernel takes the robot as an argument, and the presets share a shape: no torso offset in x or y, feet_off_x >
feet_off_y, a torso longer than wide, foot boxes far smaller than the torso, one value of each perturbation limit.  Every
entry of GEOMETRIES is the yaml preset with some fields overridden; params_of and robot_of fill the library's and the
oracle's struct from the same dict.

The state, box and pair recipes are the ones of tests/far_origin.py with the robot as a parameter (far_origin.py calls
them with its own robot); sizing() and window_classes() restate on the host what a geometry asks of the kernels: the LDS
window tile and the table tier of each box window."""
from __future__ import annotations

import functools
import math
import os
import threading

import numpy as np

import common
import oracle_py as O
from synthetic import make_map

GEOMETRIES = {
    "yaml": {},
    # the torso's pose * Pose3FromXYZ(o): R[.] * ox and R[.] * oy are multiplied by zero for both presets
    "offset": dict(torso_off_x=0.25, torso_off_y=-0.15, torso_off_z=0.1),
    # a thin long foot window (4 x 13 samples at 0.05 m)
    "plank": dict(reach_x=0.5, reach_y=0.06, reach_z=0.1),
    # windows of a cell or two; reach and wall sizes of the preprocessing of 0 or 1 cell at 0.1 m
    "tiny": dict(torso_length=0.3, torso_width=0.2, torso_height=0.1, torso_off_z=0.0, feet_off_x=0.1, feet_off_y=0.07,
                 feet_off_z=-0.15, reach_x=0.05, reach_y=0.05, reach_z=0.05),
    # wider than long, feet_off_y > feet_off_x
    "wide": dict(torso_length=0.6, torso_width=1.2, torso_height=0.25, feet_off_x=0.2, feet_off_y=0.55, reach_x=0.15,
                 reach_y=0.3, reach_z=0.3),
    # the foot diagonal exceeds the torso's: the foot sizes the window tile, the feet's 1024-triangle cap is active
    "bigfeet": dict(torso_length=0.5, torso_width=0.4, torso_height=0.2, feet_off_x=0.5, feet_off_y=0.5, reach_x=0.7,
                    reach_y=0.7, reach_z=0.3),
    "flat": dict(torso_height=0.1, reach_z=0.08),
    "tall": dict(torso_height=1.0, reach_z=0.6, feet_off_z=-0.8),
    "steep": dict(max_pitch_pert=0.35, max_roll_pert=0.2),
    "level": dict(max_pitch_pert=0.0, max_roll_pert=0.0),
}
MAPS = {"fine": (120, 0.05, 3), "coarse": (60, 0.1, 3)}

N_STATES = 8000            # OracleSampler(gm).sample(rob, SEED, FIRST, N_STATES) with the robot in question
N_BOXES = 2000             # boxes per kind: the torsos of the first 2000 states, the feet of the first 500
N_PAIRS = 1500             # draws of the edge list
SEED, FIRST = 11, 5000
PAIR_DIST = 1.5            # metres in the plane between the two ends of a pair
# a geometry whose edge verdicts leave [5 %, 95 %] at 1.5 m gets its own distance here (the robot stays as the table has it)
PAIR_DIST_OF = {
    # at 1.5 m the 0.5 m rule accepts 95.1 % of wide's pairs on the fine map (94.1 % coarse); at 2.5 m 91.1 % / 91.7 %
    "wide": 2.5,
}


def robot_of(name) -> O.Robot:
    rob = O.robot("yaml")
    for k, v in GEOMETRIES[name].items():
        assert hasattr(rob, k), k
        setattr(rob, k, v)
    return rob


def params_of(name):
    from art_planner_amd.context import make_params
    return make_params("yaml", **GEOMETRIES[name])


@functools.lru_cache(maxsize=None)
def map_of(mname):
    n, res, seed = MAPS[mname]
    return make_map(n, res, seed=seed)


# ---- the recipes, robot as a parameter (tests/far_origin.py calls these with its own robot) -------------------------------
def sample_states(gm, rob, n, seed=SEED, first=FIRST):
    """n states of the oracle's sampler on gm (cell centres in double, as the sampler forms them there)."""
    return O.OracleSampler(gm).sample(rob, seed, first, n)[0]


def details_of(gm, rob, se3):
    """The oracle's per-state detail (the five boxes' exit codes), as tests/golden/make_golden.py records it."""
    om = O.OracleMap(gm)
    return np.stack([om.state_detail(rob, s)[1] for s in se3]).astype(np.int8)


def boxes_of(gm, rob, se3):
    """(torso poses [n, 16], foot poses [4 n, 16]) of the states, in the oracle's own float arithmetic."""
    poses, _ = O.OracleMap(gm).state_poses(rob, se3)
    return poses[:, 0].reshape(-1, 16), poses[:, 1:5].reshape(-1, 16)


def pick_pairs(se3, labels, n_pairs, dist=PAIR_DIST):
    """Pairs of valid states of the list closer than dist in the plane: n_pairs draws of default_rng(2)."""
    acc = se3[labels != 0]
    rng = np.random.default_rng(2)
    ia = rng.integers(0, len(acc), n_pairs)
    pick = rng.random(n_pairs)
    ib = np.full(n_pairs, -1)
    for lo in range(0, n_pairs, 500):                       # a draw's partner: one of the valid states within dist of it
        a = acc[ia[lo:lo + 500]]
        d = np.hypot(a[:, None, 0] - acc[None, :, 0], a[:, None, 1] - acc[None, :, 1])
        d[np.arange(len(a)), ia[lo:lo + 500]] = np.inf
        near = d < dist
        cnt = near.sum(axis=1)
        k = np.minimum((pick[lo:lo + 500] * cnt).astype(int), np.maximum(cnt - 1, 0))
        order = np.argsort(~near, axis=1, kind="stable")   # the near ones first, in index order
        ib[lo:lo + 500] = np.where(cnt > 0, order[np.arange(len(a)), k], -1)
    keep = ib >= 0
    return acc[ia[keep]], acc[ib[keep]]


def edge_answers(gm, rob, a, b):
    """OracleMap's answers for a pair list: checkMotion's verdict, the lastValid pair and the 0.5 m rule with its count
    (one private OracleMap per thread; the C calls release the GIL)."""
    n = len(a)
    out = dict(ok=np.empty(n, np.uint8), lv_ok=np.empty(n, np.uint8), lv_t=np.empty(n), lv_st=np.empty((n, 7)),
               ei=np.empty(n, np.uint8), nint=np.empty(n, np.uint32))
    n_threads = max(1, min(16, len(os.sched_getaffinity(0)))) if hasattr(os, "sched_getaffinity") else 4
    chunks = np.array_split(np.arange(n), n_threads)

    def work(idx):
        if not len(idx):
            return
        om = O.OracleMap(gm)
        out["ok"][idx] = om.check_motions(rob, a[idx], b[idx])[0]
        out["lv_ok"][idx], out["lv_t"][idx], out["lv_st"][idx] = om.check_motions_last_valid(rob, a[idx], b[idx])
        out["ei"][idx], out["nint"][idx] = om.edges_interp_valid(rob, a[idx], b[idx])

    th = [threading.Thread(target=work, args=(c,)) for c in chunks]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


# ---- one list per (geometry, map), made once ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def states(name, mname):
    return sample_states(map_of(mname), robot_of(name), N_STATES)


@functools.lru_cache(maxsize=None)
def oracle_labels(name, mname):
    return common.oracle_states_valid_threaded(map_of(mname), robot_of(name), states(name, mname))


@functools.lru_cache(maxsize=None)
def oracle_details(name, mname):
    return details_of(map_of(mname), robot_of(name), states(name, mname))


@functools.lru_cache(maxsize=None)
def state_boxes(name, mname):
    """(torso poses [N_BOXES, 16], foot poses [N_BOXES, 16]): the states' own boxes."""
    torso, feet = boxes_of(map_of(mname), robot_of(name), states(name, mname)[:N_BOXES])
    return torso, feet[:N_BOXES]


@functools.lru_cache(maxsize=None)
def edge_pairs(name, mname):
    return pick_pairs(states(name, mname), oracle_labels(name, mname), N_PAIRS, PAIR_DIST_OF.get(name, PAIR_DIST))


@functools.lru_cache(maxsize=None)
def oracle_edges(name, mname):
    a, b = edge_pairs(name, mname)
    return edge_answers(map_of(mname), robot_of(name), a, b)


# ---- what a geometry asks of the kernels ---------------------------------------------------------------------------------------
def sample_spacing(n, res):
    """The height field's sample spacing of an n x n map of cell size res: len / (n - 1) in float."""
    return float(np.float32(np.float32(n * res) / (np.float32(n) - np.float32(1.0))))


def _bytes_per_wave(cand, verts, tris, tab):
    return cand + verts * 4 + tab * 4 + tris * 2


def _list_and_table(dim, cap):
    tris = (min(2 * (dim - 1) * (dim - 1), cap) + 7) & ~7
    tab = 64
    while tab < 2 * tris and tab < 4096:
        tab <<= 1
    return tris, tab


def sizing(rob, n, res):
    """size_scratch and partner_radius (csrc/artp_capi.hip) restated for an n x n map of cell size res: the window tile,
    the foot tile, the LDS sums in bytes, both partner radii (-1 = no table) and whether the upload is accepted."""
    s = sample_spacing(n, res)
    d_torso = math.sqrt(rob.torso_length ** 2 + rob.torso_width ** 2 + rob.torso_height ** 2)
    d_foot = math.sqrt(rob.reach_x ** 2 + rob.reach_y ** 2 + rob.reach_z ** 2)
    tile = max(min(int(math.ceil(max(d_torso, d_foot) / s)) + 4, n), 4)
    foot_tile = max(min(int(math.ceil(d_foot / s)) + 4, n), 4)
    verts = (tile * tile + 3) & ~3
    tris, tab = _list_and_table(tile, 4096)
    fverts = (foot_tile * foot_tile + 3) & ~3
    ftris, ftab = _list_and_table(foot_tile, 4096)
    ftris_short = min((2 * (foot_tile - 1) * (foot_tile - 1) + 7) & ~7, 1024)
    full = _bytes_per_wave(64 * 36, verts, tris, tab)
    foot_full = _bytes_per_wave(64 * 36, fverts, ftris, ftab)
    lds = dict(full=full, scan=2 * _bytes_per_wave(64 * 36, verts, min(tris, 1024), 0),
               feet=8 * _bytes_per_wave(32 * 36, fverts, ftris_short, 0),
               feet_wave=2 * _bytes_per_wave(64 * 36, fverts, ftris_short, 0), few=full + 4 * foot_full)
    limit = 160 * 1024
    accepted = tile <= 64 and lds["full"] <= limit and lds["scan"] <= limit and lds["few"] <= limit

    def radius(side):
        side = np.asarray(side, np.float32).astype(np.float64)      # RobotDev holds the sides as floats
        r = int(math.ceil(math.sqrt(float((side * side).sum())) / s)) + 3
        return -1 if r > 63 else r

    return dict(tile=tile, foot_tile=foot_tile, lds=lds, foot_list=ftris_short, partner_radius=(radius(rob.torso),
                radius(rob.foot)), accepted=accepted)


COARSE_CLASSES = ("<=7", "<=13", "<=25", ">25")          # coarse_block_exit: by the window's long side
STATS_CLASSES = ("<4", "<8", "<16", "<32", ">=32")       # table_window_stats: by its short side


def window_classes(rob, gm, se3):
    """The table tiers (csrc/pipeline.h) the boxes of the states fall into, estimated from the oracle's own box poses: a
    window is floor(extent / spacing) + 3 samples per axis, extent = the box's axis-aligned extent under its pose.
    {"torso" | "foot": {"coarse": {class: count}, "stats": {class: count}, "sides": (min short, max long)}}."""
    poses, inside = O.OracleMap(gm).state_poses(rob, se3)
    s = sample_spacing(gm.rows, gm.res)
    out = {}
    for kind, side, sl in (("torso", rob.torso, slice(0, 1)), ("foot", rob.foot, slice(1, 5))):
        P = poses[:, sl][inside[:, sl] != 0].astype(np.float64)
        side = side.astype(np.float64)
        wx = np.floor((np.abs(P[:, 4:7]) * side).sum(axis=1) / s).astype(int) + 3
        wy = np.floor((np.abs(P[:, 8:11]) * side).sum(axis=1) / s).astype(int) + 3
        long_, short = np.maximum(wx, wy), np.minimum(wx, wy)
        ci = np.digitize(long_, [8, 14, 26])
        si = np.digitize(short, [4, 8, 16, 32])
        out[kind] = dict(coarse={c: int((ci == k).sum()) for k, c in enumerate(COARSE_CLASSES) if (ci == k).any()},
                         stats={c: int((si == k).sum()) for k, c in enumerate(STATS_CLASSES) if (si == k).any()},
                         sides=(int(short.min()), int(long_.max())))
    return out
