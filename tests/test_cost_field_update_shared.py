"""What artp_field_update, artp_field_update_learned and artp_field_update_clearance share (csrc/field.h
field_update_run), on one field of each kind: the same refusals, each leaving the field as it was,
and the scratch that updates, blocks and plans allocate late or regrow between them.  test_cost_field_update.py,
test_cost_field_learned_update.py and test_cost_field_clearance_update.py hold each kind's own cases and its part of the
refusals; this file adds the rest of the matrix.  Every field covers a 40 x 40 rectangle (3 x 3 tiles, the last ones
partial) of test_cost_field_learned_update.py's map at 4 headings, with two sources: the learned kind needs that fixture's
network and cost map, the other two take the same sampler layers; its validity layers and z bounds serve plan()."""
import numpy as np
import pytest

from art_planner_amd import _capi
from lattice_ref import MOVES
from test_cost_field_clearance import CLEAR
from test_cost_field_learned import WEIGHTS, random_mask
from test_cost_field_update import bits_of, merged

pytestmark = pytest.mark.gpu

KINDS = ["plain", "learned", "clearance"]
CALL = dict(plain="update", learned="update_learned", clearance="update_clearance")
RECT = (7, 5, 40, 40)
NR, NC, N_YAW = 40, 40, 4


@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    from test_cost_field_learned_update import State
    c = Context(0, "yaml")
    s = State(c)
    s.set(1, "real", 0)
    yield s
    c.close()


def new_field(ctx, kind, mask, sources):
    """A field of the kind the way its own update test builds it."""
    if kind == "plain":
        return ctx.cost_field(mask, N_YAW, sources, rect=RECT)
    if kind == "learned":
        return ctx.learned_cost_field(mask, N_YAW, sources, rect=RECT, **WEIGHTS)
    return ctx.clearance_cost_field(mask, N_YAW, sources, rect=RECT, objective=1, **CLEAR)


def fixed_moves():
    """Every translation and rotation out of every fourth node of the rectangle that stays inside it."""
    idx = np.stack(np.meshgrid(np.arange(1, NR - 1), np.arange(1, NC - 1), np.arange(N_YAW), indexing="ij"), -1).reshape(-1, 3)[::4]
    a, b = [], []
    for m in range(10):
        t = idx.copy()
        if m < 8:
            t[:, 0] += MOVES[m][0]
            t[:, 1] += MOVES[m][1]
        else:
            t[:, 2] = (t[:, 2] + (1 if m == 8 else -1)) % N_YAW
        a.append(idx)
        b.append(t)
    return np.concatenate(a), np.concatenate(b)


def state_of(f, kind, ab):
    out = [bits_of(f.dist()), bits_of(f.edge_costs(*ab))]
    if kind == "clearance":
        out.append(f.clearance())
    return out


def same_state(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int((g != w).sum()))


# ---- 1. the refusal matrix ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_refuses_the_same_calls_and_stays_untouched(S, kind):
    ctx = S.ctx
    sources = [(10, 10, 1), (30, 5, 0)]
    mask = np.full((NR, NC), 0xf, np.uint32)
    edited = mask.copy()
    edited[20:30, 20:30] = 0                          # a valid edit: what only the kind of the call can be wrong about
    gone = edited.copy()
    gone[10, 10] = 0b1101                             # and the same without the first source's bit
    ab = fixed_moves()
    with new_field(ctx, kind, mask, sources) as f:
        before = state_of(f, kind, ab)
        own = getattr(f, CALL[kind])

        def refused(call, what):
            with pytest.raises(_capi.ArtpError) as e:
                call()
            assert e.value.status == -1, (what, e.value)
            same_state(state_of(f, kind, ab), before, what)

        for rect in [(35, 0, 10, 10), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 41, 1), (0, 39, 1, 2)]:
            refused(lambda: own(edited, rect), rect)
        refused(lambda: own(gone), "a source's bit removed")
        for other in KINDS:
            if other != kind:
                refused(lambda: getattr(f, CALL[other])(edited), other)
                refused(lambda: getattr(f, CALL[other])(edited, (15, 15, 20, 20)), other)
        sub = (15, 15, 20, 20)                        # the first source's cell lies outside: a valid update
        st = own(gone, sub)
        assert st["changed_words"] == 100 and st["removed_nodes"] == 100 * N_YAW and st["added_nodes"] == 0
        with new_field(ctx, kind, merged(mask, gone, sub), sources) as fresh:
            same_state(state_of(f, kind, ab), state_of(fresh, kind, ab), "the valid update")
            assert f.stats()["reached_nodes"] == fresh.stats()["reached_nodes"] == st["reached_nodes"]


# ---- 2. updates, blocks and a plan on one field ---------------------------------------------------------------------
def moves_of_words(words):
    """(a, b) of the moves a forward field's blocked() words stand for: bit j of node b blocks the move onto b from its
    neighbour by offset j (the rotations: j = 8 from heading k + 1, j = 9 from k - 1)."""
    a, b = [], []
    for r, c, k in np.argwhere(words != 0):
        for j in range(10):
            if (int(words[r, c, k]) >> j) & 1:
                b.append((r, c, k))
                a.append((r + MOVES[j][0], c + MOVES[j][1], k) if j < 8 else (r, c, (k + (1 if j == 8 else -1)) % N_YAW))
    return np.array(a, np.int32).reshape(-1, 3), np.array(b, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("kind", KINDS)
def test_updates_blocks_and_a_plan_share_one_fields_scratch(S, kind):
    import torch
    ctx = S.ctx
    sources = [(3, 3, 1), (35, 30, 0)]
    sub = (8, 10, 20, 20)                             # over the corner (16, 16) where four tiles meet; no source inside
    src_bits = np.zeros((NR, NC), np.uint32)
    for r, c, k in sources:
        src_bits[r, c] |= np.uint32(1 << k)
    m0 = random_mask((NR, NC), N_YAW, 61, p=0.9) | src_bits
    m1 = merged(m0, random_mask((NR, NC), N_YAW, 62, p=0.8), sub)
    m2 = random_mask((NR, NC), N_YAW, 63, p=0.9) | src_bits
    assert (m1 != m0).any() and (m2 != m1).sum() > NR * NC // 4
    m2_dev = torch.from_numpy(np.ascontiguousarray(m2.T).view(np.int32).reshape(-1)).to(f"cuda:{ctx.device}")

    with new_field(ctx, kind, m0, sources) as f:
        own = getattr(f, CALL[kind])

        def as_new(mask, what):
            """f against a new field on mask with f's blocked moves blocked."""
            words = f.blocked()
            a, b = moves_of_words(words)
            assert len(a) == f.blocked_count()
            with new_field(ctx, kind, mask, sources) as fresh:
                if len(a):
                    assert fresh.block_moves(a, b) == len(a)
                assert np.array_equal(fresh.blocked(), words), what
                want = fresh.dist()
                assert np.array_equal(bits_of(f.dist()), bits_of(want)), (what, int((bits_of(f.dist()) != bits_of(want)).sum()))
                assert f.stats()["reached_nodes"] == fresh.stats()["reached_nodes"] == int(np.isfinite(want).sum()), what
            return want

        st = own(m1, sub)                             # 1. a host mask and a rect: the staging buffer's first use
        assert st["changed_words"] == int((((m1 ^ m0) & 0xf) != 0).sum()) > 0
        d = as_new(m1, "host mask, rect")
        far = np.argwhere(np.isfinite(d) & (d >= np.quantile(d[np.isfinite(d)], 0.9)))
        targets = [tuple(int(v) for v in far[0]), tuple(int(v) for v in far[-1])]
        nodes = f.path(targets[0])[0]
        assert len(nodes) >= 4
        mid = len(nodes) // 2
        assert f.block_moves(nodes[[0, mid]], nodes[[1, mid + 1]]) == 2   # 2. the blocked words' first use
        as_new(m1, "two moves blocked")
        assert np.isinf(f.edge_costs(nodes[[0, mid]], nodes[[1, mid + 1]])).all()
        st = own(m2_dev)                              # 3. a device mask, no rect
        assert st["changed_words"] == int((((m2 ^ m1) & 0xf) != 0).sum())
        as_new(m2, "device mask")
        res = f.plan(targets)                         # 4. the plan's scratch, and the path scratch grown by it
        assert len(res) == 2 and all(r[0] in (0, 1, 2) for r in res)
        print(f"  {kind}: plan statuses {[r[0] for r in res]}, {f.blocked_count()} moves blocked, {f.plan_stats()['rounds']} rounds")
        as_new(m2, "plan")
        n_blocked = f.blocked_count()
        assert n_blocked >= 2 and f.unblock() == n_blocked                # 5. everything unblocked
        assert f.blocked_count() == 0
        as_new(m2, "unblock")
        own(m1)                                       # 6. back to the first mask
        as_new(m1, "back to the first mask")
        assert f.blocked_count() == 0 and not f.blocked().any()
