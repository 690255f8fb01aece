"""Maps far from the origin (TEST INFRASTRUCTURE; tests/test_far_origin_ref.py pins on the CPU what these inputs reach,
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
import os

import numpy as np

import common
import oracle_py as O
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
    gm = map_at(name, tuple(pos))
    return O.OracleSampler(gm).sample(O.robot(ROBOT), 11, 5000, N_SAMPLED)[0]


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
    om = O.OracleMap(map_at(name, pos))
    rob = O.robot(ROBOT)
    return np.stack([om.state_detail(rob, s)[1] for s in states(name, tuple(pos))]).astype(np.int8)


def state_boxes(name, pos, n=N_BOXES):
    """(torso poses [n, 16], foot poses [4 n, 16]) of the first n states, in the oracle's own float arithmetic."""
    om = O.OracleMap(map_at(name, pos))
    poses, _ = om.state_poses(O.robot(ROBOT), states(name, tuple(pos))[:n])
    return poses[:, 0].reshape(-1, 16), poses[:, 1:5].reshape(-1, 16)


@functools.lru_cache(maxsize=None)
def edge_pairs(name, pos):
    """Pairs of valid states of the list closer than 1.5 m in the plane: N_PAIRS draws of default_rng(2)."""
    s = states(name, tuple(pos))
    acc = s[oracle_labels(name, tuple(pos)) != 0]
    rng = np.random.default_rng(2)
    ia = rng.integers(0, len(acc), N_PAIRS)
    pick = rng.random(N_PAIRS)
    ib = np.full(N_PAIRS, -1)
    for lo in range(0, N_PAIRS, 500):                       # a draw's partner: one of the valid states within 1.5 m of it
        a = acc[ia[lo:lo + 500]]
        d = np.hypot(a[:, None, 0] - acc[None, :, 0], a[:, None, 1] - acc[None, :, 1])
        d[np.arange(len(a)), ia[lo:lo + 500]] = np.inf
        near = d < 1.5
        cnt = near.sum(axis=1)
        k = np.minimum((pick[lo:lo + 500] * cnt).astype(int), np.maximum(cnt - 1, 0))
        order = np.argsort(~near, axis=1, kind="stable")   # the near ones first, in index order
        ib[lo:lo + 500] = np.where(cnt > 0, order[np.arange(len(a)), k], -1)
    keep = ib >= 0
    return acc[ia[keep]], acc[ib[keep]]


@functools.lru_cache(maxsize=None)
def oracle_edges(name, pos):
    """OracleMap's answers for the pair list: checkMotion's verdict, the lastValid pair and the 0.5 m rule with its count
    (one private OracleMap per thread; the C calls release the GIL)."""
    import threading
    a, b = edge_pairs(name, tuple(pos))
    n = len(a)
    rob = O.robot(ROBOT)
    out = dict(ok=np.empty(n, np.uint8), lv_ok=np.empty(n, np.uint8), lv_t=np.empty(n), lv_st=np.empty((n, 7)),
               ei=np.empty(n, np.uint8), nint=np.empty(n, np.uint32))
    n_threads = max(1, min(16, len(os.sched_getaffinity(0)))) if hasattr(os, "sched_getaffinity") else 4
    chunks = np.array_split(np.arange(n), n_threads)

    def work(idx):
        if not len(idx):
            return
        om = O.OracleMap(map_at(name, pos))
        out["ok"][idx] = om.check_motions(rob, a[idx], b[idx])[0]
        out["lv_ok"][idx], out["lv_t"][idx], out["lv_st"][idx] = om.check_motions_last_valid(rob, a[idx], b[idx])
        out["ei"][idx], out["nint"][idx] = om.edges_interp_valid(rob, a[idx], b[idx])

    th = [threading.Thread(target=work, args=(c,)) for c in chunks]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def box_poses(gm, slot, side_name, seed):
    """N_BOXES random box poses around the surface of the map at its own origin (common.random_dposes)."""
    zoff = (0.42, 0.12) if side_name == "torso" else (0.0, 0.08)
    return common.random_dposes(gm, N_BOXES, np.random.default_rng(seed + 10 * slot), zoff, tilt=0.3)
