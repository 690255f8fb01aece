"""Reference for the cost-to-go fields: the lattice graph and PathLengthObjective::motionCost
restated in numpy float64, and a heapq Dijkstra over it.  Shares nothing with the library: the weights come from the
cell centres, heights and yaw bins through the objective's own formulas (path_length_objective.cpp:26-70).

Node (r, c, k) exists iff bit k of mask[r, c] is set.  Moves 0..7 go to the neighbouring cells in the order of MOVES at
the same heading, move 8 is k -> k + 1, move 9 is k -> k - 1 (mod n_yaw; none at n_yaw = 1).  Flat node index =
(r * ncols + c) * n_yaw + k."""
import heapq
from collections import deque

import numpy as np

MOVES = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def cell_centres(gm, rect=None):
    """x of every row and y of every column of the rectangle: grid_map's getPosition, as the sampler computes it."""
    r0, c0, nr, nc = rect if rect is not None else (0, 0, gm.rows, gm.cols)
    res = gm.len_x / gm.rows
    x = (gm.pos_x + (0.5 * gm.len_x - 0.5 * res)) + res * -np.arange(r0, r0 + nr, dtype=np.float64)
    y = (gm.pos_y + (0.5 * gm.len_y - 0.5 * res)) + res * -np.arange(c0, c0 + nc, dtype=np.float64)
    return x, y


def yaw_bins(n_yaw):
    yaw = (2.0 * np.pi / n_yaw) * np.arange(n_yaw, dtype=np.float64)
    return np.where(yaw > np.pi, yaw - 2.0 * np.pi, yaw)


def angle_diff(x, y):
    d = np.abs(y - x)
    return np.where(d > np.pi, 2.0 * np.pi - d, d)


class Lattice:
    def __init__(self, mask, n_yaw, x, y, z, objective=1, max_lon_vel=0.5, max_lat_vel=0.1, max_ang_vel=0.5):
        mask = np.asarray(mask, np.uint32)
        self.nr, self.nc = mask.shape
        self.n_yaw = int(n_yaw)
        self.shape = (self.nr, self.nc, self.n_yaw)
        self.bits = ((mask[..., None] >> np.arange(self.n_yaw, dtype=np.uint32)) & 1).astype(bool)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        z = np.asarray(z, np.float32).astype(np.float64)
        assert x.shape == (self.nr,) and y.shape == (self.nc,) and z.shape == (self.nr, self.nc)
        yaw = yaw_bins(self.n_yaw)
        cy, sy = np.cos(yaw), np.sin(yaw)
        # w[m][r, c, k]: motionCost((r, c, k) -> its neighbour by move m); +inf where the edge does not exist
        self.w = np.full((10,) + self.shape, np.inf)
        for m, (dr, dc) in enumerate(MOVES):
            a = (slice(max(0, -dr), self.nr - max(0, dr)), slice(max(0, -dc), self.nc - max(0, dc)))
            b = (slice(max(0, dr), self.nr - max(0, -dr)), slice(max(0, dc), self.nc - max(0, -dc)))
            x_dif = (x[b[0]] - x[a[0]])[:, None, None]
            y_dif = (y[b[1]] - y[a[1]])[None, :, None]
            z_dif = (z[b] - z[a])[..., None]
            if objective == 0:
                cost = np.sqrt(x_dif * x_dif + y_dif * y_dif + z_dif * z_dif) / max_lon_vel + 0.0 * yaw
            else:
                lon = cy * x_dif + sy * y_dif
                lat = -sy * x_dif + cy * y_dif
                t_yaw = np.abs(angle_diff(yaw, yaw)) / max_ang_vel
                cost = np.maximum(np.maximum(np.abs(lon) / max_lon_vel, np.abs(lat) / max_lat_vel), t_yaw)
                cost = cost + 0.0 * z_dif
            ok = self.bits[a] & self.bits[b] & np.isfinite(cost)
            self.w[m][a] = np.where(ok, cost, np.inf)
        if self.n_yaw > 1:
            for m, step in ((8, 1), (9, -1)):
                k2 = (np.arange(self.n_yaw) + step) % self.n_yaw
                if objective == 0:
                    cost = np.zeros(self.n_yaw)   # the same x, y, z: sqrt(0) / max_lon_vel
                else:
                    cost = np.abs(angle_diff(yaw[k2], yaw)) / max_ang_vel   # lon = lat = 0
                ok = self.bits & self.bits[..., k2]
                self.w[m] = np.where(ok, cost[None, None, :], np.inf)
        self._csr = {}

    def index(self, node):
        r, c, k = node
        return (int(r) * self.nc + int(c)) * self.n_yaw + int(k)

    def exists(self, node):
        r, c, k = node
        return 0 <= r < self.nr and 0 <= c < self.nc and 0 <= k < self.n_yaw and bool(self.bits[r, c, k])

    def neighbour_index(self, m):
        """Flat index of every node's neighbour by move m (garbage where the edge does not exist)."""
        idx = np.arange(self.nr * self.nc * self.n_yaw, dtype=np.int64).reshape(self.shape)
        if m < 8:
            return idx + (MOVES[m][0] * self.nc + MOVES[m][1]) * self.n_yaw
        k = np.arange(self.n_yaw)
        return idx - k + (k + (1 if m == 8 else -1)) % self.n_yaw

    def csr(self, reverse):
        """Adjacency in the direction the search expands: forward u -> its successors with w(u -> v); reverse v -> the
        nodes a that have an edge a -> v, with w(a -> v)."""
        if reverse in self._csr:
            return self._csr[reverse]
        n = self.nr * self.nc * self.n_yaw
        src, dst, wt = [], [], []
        for m in range(10):
            w = self.w[m].reshape(-1)
            e = np.flatnonzero(np.isfinite(w))
            a, b = e, self.neighbour_index(m).reshape(-1)[e]
            src.append(b if reverse else a)
            dst.append(a if reverse else b)
            wt.append(w[e])
        src, dst, wt = np.concatenate(src), np.concatenate(dst), np.concatenate(wt)
        order = np.argsort(src, kind="stable")
        indptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=n), out=indptr[1:])
        out = (indptr.tolist(), dst[order].tolist(), wt[order].tolist())
        self._csr[reverse] = out
        return out

    def dijkstra(self, sources, reverse=False):
        """(dist, hops), both (nrows, ncols, n_yaw): the smallest left-fold cost from any source (reverse: to any source,
        folded from the source end outwards) and the edges of the path that gave it; +inf / -1 where there is none."""
        n = self.nr * self.nc * self.n_yaw
        indptr, adj, wt = self.csr(bool(reverse))
        dist = [float("inf")] * n
        hops = [-1] * n
        done = [False] * n
        heap = []
        for s in sources:
            assert self.exists(s), s
            i = self.index(s)
            dist[i], hops[i] = 0.0, 0
            heap.append((0.0, i))
        heapq.heapify(heap)
        while heap:
            d, u = heapq.heappop(heap)
            if done[u]:
                continue
            done[u] = True
            for e in range(indptr[u], indptr[u + 1]):
                v = adj[e]
                nd = d + wt[e]
                if nd < dist[v]:
                    dist[v] = nd
                    hops[v] = hops[u] + 1
                    heapq.heappush(heap, (nd, v))
        return np.array(dist).reshape(self.shape), np.array(hops, np.int64).reshape(self.shape)

    def components(self):
        """Label of the connected component of every node (-1 = not a node), by flood fill over the moves; and the sizes."""
        n = self.nr * self.nc * self.n_yaw
        indptr, adj, _ = self.csr(False)
        label = [-1] * n
        exists = self.bits.reshape(-1).tolist()
        sizes = []
        for s in range(n):
            if not exists[s] or label[s] >= 0:
                continue
            lab = len(sizes)
            label[s] = lab
            q = deque([s])
            cnt = 0
            while q:
                u = q.popleft()
                cnt += 1
                for e in range(indptr[u], indptr[u + 1]):
                    v = adj[e]
                    if label[v] < 0:
                        label[v] = lab
                        q.append(v)
            sizes.append(cnt)
        return np.array(label, np.int64).reshape(self.shape), np.array(sizes, np.int64)

    def move_between(self, a, b):
        """The move 0..9 that leads from node a to node b, or None."""
        (r, c, k), (r2, c2, k2) = a, b
        if k == k2 and (r2 - r, c2 - c) in MOVES:
            return MOVES.index((r2 - r, c2 - c))
        if (r, c) == (r2, c2) and self.n_yaw > 1:
            if k2 == (k + 1) % self.n_yaw:
                return 8
            if k2 == (k - 1) % self.n_yaw:
                return 9
        return None
