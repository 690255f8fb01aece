"""Reference for the blocked-move set of a cost-to-go field: a blocked move is an absent edge, so the
restatement is lattice_ref.Lattice with w[m][a] = +inf for every blocked move a -> b, and the repair is
field_update_ref.update on an unchanged mask: unsupport, relax, hop reset, unsupport, relax.  Shares nothing with the
library; tests/test_field_plan_ref.py holds it against lattice_ref's Dijkstra on the blocked weights.

words() restates the layout of artp_field_blocked: one 16-bit word per node, bit j of node v = pull slot (v, j); a forward
field stores the move a -> b at its END b under the offset that leads back, a reverse field at its START a under the move.  At two headings a rotation is
moves 8 and 9 at once: both weights go, both bits are set, and it counts as one move."""
import numpy as np

import field_update_ref as FU


def back_move(m):
    return 7 - m if m < 8 else (9 if m == 8 else 8)


def move_of(lat, a, b):
    m = lat.move_between(tuple(int(v) for v in a), tuple(int(v) for v in b))
    assert m is not None, (a, b)
    return m


def slots_of(lat, m):
    """The moves that hold the same edge as move m: at two headings k + 1 and k - 1 are one neighbour, so a rotation is
    both move 8 and move 9 (Lattice.w carries it twice)."""
    return (8, 9) if lat.n_yaw == 2 and m >= 8 else (m,)


def set_weights(lat, moves, value):
    """w(a -> b) = value for every move; value(m, a) when callable.  The adjacency cache goes."""
    for a, b in moves:
        for m in slots_of(lat, move_of(lat, a, b)):
            lat.w[m][tuple(int(v) for v in a)] = value(m, a) if callable(value) else value
    lat._csr.clear()


def block(lat, moves):
    """The blocked moves become absent edges; returns the weights they had, for unblock()."""
    saved = [(a, b, float(lat.w[move_of(lat, a, b)][tuple(int(v) for v in a)])) for a, b in moves]
    set_weights(lat, moves, np.inf)
    return saved


def unblock(lat, saved):
    for a, b, w in saved:
        set_weights(lat, [(a, b)], w)


def words(shape, lat, moves, reverse):
    """(nrows, ncols, n_yaw) uint16 as artp_field_blocked gives them for this set of moves."""
    out = np.zeros(shape, np.uint16)
    for a, b in moves:
        for m in slots_of(lat, move_of(lat, a, b)):
            owner, j = (a, m) if reverse else (b, back_move(m))
            out[tuple(int(v) for v in owner)] |= np.uint16(1 << j)
    return out


def repair(lat, dist, hops, reverse=False, hop_rule=True):
    """(dist, hops, stats) of a field after the weights of lat changed under it: the passes of artp_field_update on an
    unchanged mask.  Exact for weights that rose (a block) and for weights that fell (an unblock)."""
    return FU.update(lat, lat.bits, dist, hops, reverse, hop_rule)
