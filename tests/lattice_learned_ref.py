"""Reference for the learned-cost fields: a heapq Dijkstra over an EXPLICIT per-edge weight array,
which need not be symmetric, on lattice_ref's nodes and moves; and the pieces a test needs to make that array outside the
library: the EdgeMatrix row of every move from the lattice poses, and MotionCostObjective's pricing of one sub-edge in
numpy float64.

w[m][r, c, k] is the cost of move m FROM node (r, c, k).  An edge exists iff both ends are nodes of the mask inside the
rectangle and its weight is neither negative nor NaN nor +inf; a weight of 0 is an edge."""
from collections import deque

import numpy as np

import lattice_ref as LR


class LearnedLattice(LR.Lattice):
    def __init__(self, mask, n_yaw, w):
        nr, nc = np.asarray(mask).shape
        # the geometry is not used: on a flat lattice of coincident cells every weight of the base class is finite, so its
        # w is finite exactly where both ends of the move exist
        super().__init__(mask, n_yaw, np.zeros(nr), np.zeros(nc), np.zeros((nr, nc)), objective=1)
        w = np.asarray(w, np.float64)
        assert w.shape == self.w.shape, (w.shape, self.w.shape)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(self.w) & (w >= 0.0)        # NaN compares false
        self.w = np.where(ok, w, np.inf)
        self._csr = {}

    def bfs_depth(self, sources, reverse=False):
        """Edges of the shortest chain of existing edges from any source (reverse: to any source); -1 where there is none."""
        indptr, adj, _ = self.csr(bool(reverse))
        depth = [-1] * (self.nr * self.nc * self.n_yaw)
        q = deque()
        for s in sources:
            depth[self.index(s)] = 0
            q.append(self.index(s))
        while q:
            u = q.popleft()
            for e in range(indptr[u], indptr[u + 1]):
                v = adj[e]
                if depth[v] < 0:
                    depth[v] = depth[u] + 1
                    q.append(v)
        return np.array(depth, np.int64).reshape(self.shape)


def yaw_of_quat(q):
    """roadmap.h yaw_from_quat on (..., 4) quaternions x y z w: float64 arithmetic, the result rounded to float32."""
    x, y, z, w = (q[..., i] for i in range(4))
    return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)).astype(np.float32)


def move_slices(nr, nc, m):
    """(a, b): the index slices of the start cells of translation move m whose target lies inside, and of those targets."""
    dr, dc = LR.MOVES[m]
    a = (slice(max(0, -dr), nr - max(0, dr)), slice(max(0, -dc), nc - max(0, dc)))
    b = (slice(max(0, dr), nr - max(0, -dr)), slice(max(0, dc), nc - max(0, -dc)))
    return a, b


def edge_rows(poses):
    """rows[m][r, c, k] = the EdgeMatrix row of move m from (r, c, k): target (x, y, yaw) then start (x, y, yaw), float32,
    from poses (nrows, ncols, n_yaw, 7); zeros where the move leaves the rectangle (inside[m] is False there)."""
    nr, nc, n_yaw = poses.shape[:3]
    xyw = np.stack([poses[..., 0].astype(np.float32), poses[..., 1].astype(np.float32), yaw_of_quat(poses[..., 3:7])], -1)
    rows = np.zeros((10, nr, nc, n_yaw, 6), np.float32)
    inside = np.zeros((10, nr, nc, n_yaw), bool)
    for m in range(8):
        a, b = move_slices(nr, nc, m)
        rows[m][a][..., 0:3] = xyw[b]
        rows[m][a][..., 3:6] = xyw[a]
        inside[m][a] = True
    if n_yaw > 1:
        for m, step in ((8, 1), (9, -1)):
            k2 = (np.arange(n_yaw) + step) % n_yaw
            rows[m][..., 0:3] = xyw[:, :, k2]
            rows[m][..., 3:6] = xyw
            inside[m] = True
    return rows, inside


def price(cost3, w_energy, w_time, w_risk, risk_threshold):
    """chain_motion_cost_kernel on a chain of one sub-edge: (..., 3) float32 (energy, time, risk) -> float64 cost; the
    weights and the threshold are floats widened to f64; +inf where the risk exceeds the threshold."""
    c = np.asarray(cost3, np.float32).astype(np.float64)
    en, ti, ri = c[..., 0], c[..., 1], c[..., 2]
    we, wt, wr, thr = (np.float64(np.float32(v)) for v in (w_energy, w_time, w_risk, risk_threshold))
    with np.errstate(invalid="ignore"):
        total = 0.0 + ((en * we + ti * wt) + ri * wr)
        return np.where(ri <= thr, total, np.inf)
