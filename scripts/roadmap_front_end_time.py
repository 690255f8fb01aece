"""Host-side timings of the roadmap and map-preprocessing front ends: the statements of bench.py's roadmap_n1 and
preprocess_n2 sections (--full) on their own, so that two builds can be compared in a minute.  One JSON line.
Usage: python scripts/roadmap_front_end_time.py [TREE]
TREE = the checkout whose art_planner_amd package (and the libartp.so built in it) is measured; default: this one.
profiles/roadmap_front_end_owned.txt: the parent commit's checkout and this one, alternating, three processes each."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path[:0] = [tree, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from art_planner_amd.context import Context  # noqa: E402
from art_planner_amd.roadmap import Roadmap  # noqa: E402
from art_planner_amd import _capi  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

assert os.path.abspath(_capi.LIB_PATH).startswith(tree), _capi.LIB_PATH
seed = 42
ctx = Context(0, "yaml")
gm = map_from_device(ctx, raw_map(400, 0.04, seed=1234))
probe = ctx.sample_states(seed, 9_000_000, 1 << 15)
okp = probe[ctx.validate_states(probe) != 0]
s_state = okp[np.argmin(np.hypot(okp[:, 0] - (gm.pos_x - 0.4 * gm.len_x), okp[:, 1] - (gm.pos_y - 0.4 * gm.len_y)))]
g_state = okp[np.argmin(np.hypot(okp[:, 0] - (gm.pos_x + 0.4 * gm.len_x), okp[:, 1] - (gm.pos_y + 0.4 * gm.len_y)))]
roadmap = {}
for n_m in (10_000, 100_000):
    Roadmap(ctx, s_state, g_state, n_milestones=1000, seed=seed).close()
    t0 = time.perf_counter()
    rm = Roadmap(ctx, s_state, g_state, n_milestones=n_m, seed=seed)
    t1 = time.perf_counter()
    path, cost, rep = rm.solve()
    t2 = time.perf_counter()
    st = rm.stats()
    t3 = time.perf_counter()
    rm.revalidate()
    t4 = time.perf_counter()
    rm.solve()
    t5 = time.perf_counter()
    rm.close()
    roadmap[f"milestones_{n_m}"] = {"build_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3,
                                     "revalidate_ms": (t4 - t3) * 1e3, "resolve_ms": (t5 - t4) * 1e3,
                                     "path_cost_s": repr(cost), "lazy_removals": rep,
                                     "candidate_edges": int(st["candidate_edges"])}
for name, kw in (("prm_motion_cost_order", dict(n_milestones=10_000, max_n_edges=50_000, construction=1)),
                 ("lazy_prm_star_order_10000", dict(n_milestones=10_000, construction=2))):
    for attempt in ("first", "steady"):
        t0 = time.perf_counter()
        rm = Roadmap(ctx, s_state, g_state, seed=seed, **kw)
        t1 = time.perf_counter()
        path, cost, rep = rm.solve()
        t2 = time.perf_counter()
        rm.close()
    roadmap[name] = {"build_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3, "path_cost_s": repr(cost),
                     "lazy_removals": rep}
pre_ms, inst_new, inst_patch, inst_same = [], [], [], []
other = raw_map(400, 0.04, seed=4321)
e_a, e_b = gm["elevation"], other["elevation"]
e_p = e_a.copy()
e_p[180:220, 150:190] += np.float32(0.05)


def one(elev, trav, sink):
    t0 = time.perf_counter()
    pp = ctx.preprocess_map(elev, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y, traversability=trav)
    t1 = time.perf_counter()
    pp.install()
    ctx.synchronize()
    t2 = time.perf_counter()
    pp.close()
    pre_ms.append((t1 - t0) * 1e3)
    sink.append((t2 - t1) * 1e3)


for r_ in range(5):
    one(e_b if r_ % 2 == 0 else e_a, other["traversability"] if r_ % 2 == 0 else gm["traversability"], inst_new)
one(e_a, gm["traversability"], [])
for r_ in range(5):
    one(e_p if r_ % 2 == 0 else e_a, gm["traversability"], inst_patch)
one(e_a, gm["traversability"], [])
for r_ in range(5):
    one(e_a, gm["traversability"], inst_same)
preprocess = {"preprocess_ms_incl_h2d": float(np.median(pre_ms)), "install_ms_incl_tables": float(np.median(inst_new)),
              "reinstall_ms_40x40_patch_changed": float(np.median(inst_patch)),
              "reinstall_ms_identical_map": float(np.median(inst_same))}
ctx.close()
print(json.dumps({"tree": tree, "roadmap_n1": roadmap, "preprocess_n2": preprocess}))
