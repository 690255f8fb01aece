"""Maps far from the origin (TEST INFRASTRUCTURE; the recipes are those of tests/robot_geometry.py with the yaml robot;
tests/test_far_origin_ref.py pins on the CPU what these inputs reach,
tests/test_far_origin.py runs them on the GPU).

An elevation map is centred on the robot, so its position is wherever odometry puts it.  The reference forms world-frame
float coordinates at exactly these points (Pose3FromSE3's float pose, ODE's box origin minus the height field's
position, the cell centres of the normal estimate), so the rounding of a coordinate -- 2.4e-4 m at 2 km, 8 mm at 77 km,
0.5 m at a UTM northing -- decides labels there, and the oracle does the same float arithmetic.

Layers are made ONCE, at origin zero, and `moved` only changes the position: a difference between two origins is then the
arithmetic of the code under test and nothing else.  Every comparison is made AT the origin in question, against the
oracle or a restatement fed that origin; nothing is shifted back to origin zero."""
from __future__ import annotations

import copy
import functools

import numpy as np

import common
import oracle_py as O
import robot_geometry as RG
import sampler_probe
from synthetic import make_map

ORIGINS = {"odom": (137.3, -58.9), "km": (-2048.25, 1023.75), "far": (42000.123, -77000.456),
           "utm": sampler_probe.ORIGINS["utm"]}
ZERO = (0.0, 0.0)
MAPS = {"p160": (160, 0.04, 7), "p120": (120, 0.05, 3)}
ROBOT = "yaml"

N_SAMPLED = 20000          # OracleSampler(gm).sample(rob, 11, 5000, N_SAMPLED) at the origin in question
N_BOXES = 5000             # states whose boxes the exit-code mix is counted on; dposes per (slot, box kind)
N_PAIRS = 4000             # draws of the edge list


@functools.lru_cache(maxsize=None)
def base_map(name):
    n, res, seed = MAPS[name]
    return make_map(n, res, seed=seed)


def moved(gm, pos):
    """A shallow copy: the same layer arrays at another position."""
    out = copy.copy(gm)
    out.layers = dict(gm.layers)
    out.pos_x, out.pos_y = float(pos[0]), float(pos[1])
    return out


def map_at(name, pos):
    return moved(base_map(name), pos)


@functools.lru_cache(maxsize=None)
def states(name, pos):
    """The state list: 20 000 states of the oracle's sampler on the map at pos (cell centres in double, as the sampler
    forms them there).  The same (seed, index) picks the same cell at every origin, so states(name, ZERO) is the same
    list in the frame of origin zero."""
    return RG.sample_states(map_at(name, tuple(pos)), O.robot(ROBOT), N_SAMPLED)


def random_moved_states(name, pos, n=N_SAMPLED, seed=5):
    """common.random_states of the map at origin zero, moved with the map."""
    rs = common.random_states(base_map(name), n, np.random.default_rng(seed))
    rs[:, 0] += float(pos[0])
    rs[:, 1] += float(pos[1])
    return rs


@functools.lru_cache(maxsize=None)
def oracle_labels(name, pos):
    return common.oracle_states_valid_threaded(map_at(name, pos), O.robot(ROBOT), states(name, tuple(pos)))


@functools.lru_cache(maxsize=None)
def oracle_details(name, pos):
    """The oracle's per-state detail (the five boxes' exit codes), as tests/golden/make_golden.py records it."""
    return RG.details_of(map_at(name, pos), O.robot(ROBOT), states(name, tuple(pos)))


def state_boxes(name, pos, n=N_BOXES):
    """(torso poses [n, 16], foot poses [4 n, 16]) of the first n states, in the oracle's own float arithmetic."""
    return RG.boxes_of(map_at(name, pos), O.robot(ROBOT), states(name, tuple(pos))[:n])


@functools.lru_cache(maxsize=None)
def edge_pairs(name, pos):
    """Pairs of valid states of the list closer than 1.5 m in the plane: N_PAIRS draws of default_rng(2)."""
    return RG.pick_pairs(states(name, tuple(pos)), oracle_labels(name, tuple(pos)), N_PAIRS, 1.5)


@functools.lru_cache(maxsize=None)
def oracle_edges(name, pos):
    """OracleMap's answers for the pair list: checkMotion's verdict, the lastValid pair and the 0.5 m rule with its count."""
    a, b = edge_pairs(name, tuple(pos))
    return RG.edge_answers(map_at(name, pos), O.robot(ROBOT), a, b)


def box_poses(gm, slot, side_name, seed):
    """N_BOXES random box poses around the surface of the map at its own origin (common.random_dposes)."""
    zoff = (0.42, 0.12) if side_name == "torso" else (0.0, 0.08)
    return common.random_dposes(gm, N_BOXES, np.random.default_rng(seed + 10 * slot), zoff, tilt=0.3)
