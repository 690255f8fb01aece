"""What a roadmap derives from its edge arrays -- the adjacency, the cache of motion verdicts, the device graph, the resident
endpoint states (csrc/roadmap.h: roadmap_edges_changed / roadmap_weights_changed / roadmap_remove_edge) -- is invalidated
wherever the arrays change: two roadmaps built alike go through the same calls, one of them with extra calls in between
that must not change any answer, and agree bit for bit after every step.  No tolerance: two runs of one library.

Map and query of test_scratch_balance.py (make_map(100, 0.1, seed=5), 200 milestones, seed 5), path-length objective,
constructions 0, 1 and 2.  On this grid the lazy path check does remove edges with seed 5 (construction 2: 282, 1 and 291
removals in the three solves of the far queries, which 200 milestones do not connect; construction 0: 2 removals on the
way to the 4-state path of the closing query, whose goal is a vertex the start does reach): the sequence counts removals
and path states per solve, and test_lazy_removals_and_paths_happened fails if no construction had a removal or a path.

The error paths that do not need a failing device are here as well: an invalid start or goal is refused with the message
it always had and leaves the roadmap as it was."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import shortest_path

pytestmark = pytest.mark.gpu

REPLANS = {}  # construction -> (lazy removals, path states) of the shared solves of a sequence that passed


@pytest.fixture(scope="module")
def setup():
    from art_planner_amd.context import Context
    from synthetic import make_map
    gm = make_map(100, 0.1, seed=5)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    se3 = ctx.sample_states(99, 0, 1 << 14)
    ok = ctx.validate_states(se3) != 0
    cand, invalid = se3[ok], se3[~ok]
    assert len(cand) >= 8 and len(invalid) >= 1

    def near(x, y, skip=0):
        return cand[np.argsort(np.hypot(cand[:, 0] - x, cand[:, 1] - y), kind="stable")[skip]]

    start, goal = near(gm.pos_x - 3.5, gm.pos_y - 3.5), near(gm.pos_x + 3.5, gm.pos_y + 3.5)
    others = cand[np.linspace(0, len(cand) - 1, 6).astype(int)]
    near_goal = near(start[0], start[1], skip=1)  # the valid sample next to the start: inside its neighbour list
    yield gm, ctx, start, goal, others, near_goal, invalid[0]
    ctx.close()


def _build(ctx, start, goal, construction):
    from art_planner_amd.roadmap import Roadmap
    return Roadmap(ctx, start, goal, n_milestones=200, seed=5, construction=construction, objective=0)


def _state(rm):
    d = rm.export()
    d["stats"] = np.array(sorted((k, int(v)) for k, v in rm.stats().items()), dtype=object)
    return d


def _assert_same_state(a, b, where):
    sa, sb = _state(a), _state(b)
    assert list(sa["stats"].tolist()) == list(sb["stats"].tolist()), where
    for f in sa:
        if f == "stats":
            continue
        assert sa[f].shape == sb[f].shape and sa[f].tobytes() == sb[f].tobytes(), (where, f)


def _assert_same_answer(ra, rb, where):
    (pa, ca, na), (pb, cb, nb) = ra, rb
    assert (pa is None) == (pb is None), where
    if pa is not None:
        assert pa.shape == pb.shape and pa.tobytes() == pb.tobytes(), where
    assert np.float64(ca).tobytes() == np.float64(cb).tobytes() and na == nb, (where, ca, cb, na, nb)


def _sequence(setup, construction):
    """the shared sequence on A and B with A's extra calls; the removals A's shared solves reported (run once)"""
    if construction in REPLANS:
        return REPLANS[construction]
    gm, ctx, start, goal, others, near_goal, _ = setup
    A, B, C = (_build(ctx, start, goal, construction) for _ in range(3))
    try:
        _assert_same_state(A, B, "built")
        # the near goal's answer on an untouched third roadmap: set_query + solve
        C.set_query(start, near_goal)
        near_ref = C.solve()
        # 200 milestones do not connect the far corners of this map, so the sequence ends with a goal that the start does
        # reach: the state of the vertex the most valid edges away from it in the graph as built (the smallest id of those)
        C.set_query(start, goal)
        d = C.export()
        keep = d["edge_valid"] != 0
        E = d["edges"][keep].astype(np.int64)
        nv = len(d["verts"])
        hops = shortest_path(csr_matrix((np.ones(len(E)), (E[:, 0], E[:, 1])), shape=(nv, nv)), directed=False,
                             unweighted=True, indices=0)
        hops[~np.isfinite(hops)] = -1
        hops[:2] = -1
        reached = d["verts"][int(np.argmax(hops))].copy() if hops.max() >= 1 else near_goal  # (a start without edges)

        def near_many(where):
            """A only: one goal next to the start goes through set_query + solve on A itself, A's query prefix is
            snapshotted and restored; the answer is the third roadmap's and A is what it was"""
            before = _state(A)
            out = A.solve_many(start, near_goal[None, :])
            assert out["stats"]["fallback"] == 1, (where, out["stats"])
            assert out["status"][0] == (0 if near_ref[0] is not None else 2), where
            if near_ref[0] is not None:
                assert out["paths"][0].tobytes() == near_ref[0].tobytes(), where
                assert out["cost"][0].tobytes() == np.float64(near_ref[1]).tobytes(), where
            after = _state(A)
            for f in before:
                if f != "stats":
                    assert before[f].tobytes() == after[f].tobytes(), (where, f)

        replans = []

        def both_solve(where, again):
            ra, rb = A.solve(), B.solve()
            print(f"construction {construction} {where}: near goal {'reached' if near_ref[0] is not None else 'not reached'}, cost {ra[1]!r}, {ra[2]} removals, "
                  f"{None if ra[0] is None else len(ra[0])} states")
            _assert_same_answer(ra, rb, where)
            _assert_same_state(A, B, where)
            replans.append((ra[2], 0 if ra[0] is None else len(ra[0])))
            if again:  # A only: the same path and cost once more, nothing left to remove, nothing changed
                r2 = A.solve()
                _assert_same_answer((ra[0], ra[1], 0), r2, where + ", repeated")
                _assert_same_state(A, B, where + ", repeated")

        near_many("before the first solve")   # restore must leave no adjacency of the near query behind
        both_solve("first solve", again=True)
        for rm in (A, B):
            rm.set_query(others[0], others[1])
        _assert_same_state(A, B, "set_query to the second pair")
        both_solve("solve of the second pair", again=False)
        near_many("before the first revalidate")
        ia, ib = A.revalidate(), B.revalidate()
        assert ia == ib
        _assert_same_state(A, B, "revalidate")
        assert A.revalidate() == ia            # A only: straight again, on the unchanged map
        _assert_same_state(A, B, "revalidate, repeated")
        near_many("after the revalidates")
        assert A.revalidate() == ia            # ... and once more behind a restored query prefix
        _assert_same_state(A, B, "revalidate behind solve_many")
        ga, gb = A.grow(50), B.grow(50)
        assert ga == gb and A.stats()["vertices"] > 200
        _assert_same_state(A, B, "grow by 50")
        for rm in (A, B):
            rm.set_query(start, goal)
        _assert_same_state(A, B, "set_query back")
        # stale edge states, and more edges than the resident block was sized for
        ia, ib = A.revalidate(), B.revalidate()
        assert ia == ib
        _assert_same_state(A, B, "revalidate of the grown roadmap")
        both_solve("last solve", again=True)
        for rm in (A, B):
            rm.set_query(start, reached)
        _assert_same_state(A, B, "set_query to a state in reach")
        both_solve("solve of the pair in reach", again=True)
        REPLANS[construction] = replans
        return replans
    finally:
        for rm in (A, B, C):
            rm.close()


@pytest.mark.parametrize("construction", [0, 1, 2])
def test_extra_calls_between_the_steps_change_no_answer(setup, construction):
    assert len(_sequence(setup, construction)) == 4


def test_lazy_removals_and_paths_happened(setup):
    """the precondition of the test above: somewhere in the sequences a solve removed edges (else the removal path of
    the derived state was never taken on this grid, and the seed has to change), and somewhere a path was found (else
    no path was ever compared)"""
    replans = {c: _sequence(setup, c) for c in (0, 1, 2)}
    print("(lazy removals, path states) per construction and solve:", replans)
    assert any(n > 0 for r in replans.values() for n, _ in r), replans
    assert any(m >= 3 for r in replans.values() for _, m in r), replans


def test_invalid_queries_are_refused_with_their_messages(setup):
    from art_planner_amd import _capi
    gm, ctx, start, goal, others, _, invalid = setup
    with pytest.raises(_capi.ArtpError) as e:
        _build(ctx, invalid, goal, 0)
    assert e.value.status == -1 and "start state is not valid" in str(e.value)
    for construction in (0, 1, 2):
        rm = _build(ctx, start, goal, construction)
        try:
            before = _state(rm)
            with pytest.raises(_capi.ArtpError) as e:
                rm.set_query(others[0], invalid)
            assert e.value.status == -1 and "goal state is not valid" in str(e.value)
            after = _state(rm)
            for f in before:
                if f != "stats":
                    assert before[f].tobytes() == after[f].tobytes(), (construction, f)
            # the map changes under the start: a block of terrain, both layers, like a new obstacle
            ix = int((gm.pos_x + 0.5 * gm.len_x - start[0]) / gm.res)
            iy = int((gm.pos_y + 0.5 * gm.len_y - start[1]) / gm.res)
            r0, c0 = max(ix - 6, 0), max(iy - 6, 0)
            for slot, name in ((0, "elevation"), (1, "elevation_masked")):
                patch = gm[name][r0:r0 + 12, c0:c0 + 12]
                if slot == 0:
                    patch = np.where(np.isfinite(patch), patch, np.float32(0)) + np.float32(0.6)
                else:
                    patch = np.full_like(patch, -np.inf)
                ctx.update_layer_rect(slot, np.asfortranarray(patch), r0, c0)
            try:
                assert ctx.validate_states(start[None, :])[0] == 0
                with pytest.raises(_capi.ArtpError) as e:
                    rm.grow(50)
                assert e.value.status == -1 and "start state is not valid" in str(e.value)
                after = _state(rm)
                assert list(before["stats"].tolist()) == list(after["stats"].tolist())
                for f in before:
                    if f != "stats":
                        assert before[f].tobytes() == after[f].tobytes(), (construction, f)
            finally:
                ctx.upload_map(gm)
        finally:
            rm.close()
