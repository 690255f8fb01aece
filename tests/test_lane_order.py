"""Writers of state the lanes share, against a reader still in flight on another lane.

Every case: lane 1 runs on a torch stream.  A filler with a result known in advance (lane_busy.py) is queued on that
stream, the reader R behind it.  Lane 0 then calls the writer W at once, and lane 1 the reader again (R') with no host wait
in between; one synchronize() ends the run.  R must be the result under the OLD state (W may not overtake it), R' the
result under the NEW state (it may not run ahead of W).  Both expected results come from a sequential run of the same
calls with a host wait after each, and that run is tied to the CPU oracles.  Old and new results differ in at least a
tenth of their elements, or the two orders could not be told apart.

The filler runs for ten times the longest host time any writer took in the sequential runs (lanes idle), 0.2 s at the
most: the machines are shared, and a descheduled issuing thread stretches the host time.  A case only counts if lane 1's
stream was still busy immediately before W -- and, for the writers that return with their device work queued,
immediately after W as well.  Both lanes run on torch streams, and lane 1's is chosen so that the device runs it side by
side with lane 0's (lane_busy.Busy.concurrent_stream): streams that share a hardware queue run in the order they were
fed, and a library without the ordering passed the first version of this test that way.

artp_preprocessed_install of a map of the same geometry is NOT among those: its layer step compares the new layer with
the installed one and reads the answer back through a wait on the lane's stream, which by then stands behind the other
lanes' work (order_after_other_lanes), and its sampler step and z bounds wait for the stream again.  The call returns
after lane 1's filler and R have run, so the condition "still busy after W" cannot hold for it; the case keeps the
condition before W and both results.  Likewise one update_layer_rects call is asynchronous, a second one waits for the
first one's staging copy: the case writes one slot in one call."""
import os
import sys
import time

import numpy as np
import pytest

import common
import oracle_py as O
import preprocess_restated as P
from lane_busy import CEILING_S, Busy
from synthetic import GridMap

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import motion_cost_oracle as mo  # noqa: E402
import convert_weights as cw  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 4096
ROWS, COLS, RES = 97, 61, 0.04
POS = (0.7, -0.3)
GEOM = (ROWS * RES, COLS * RES) + POS
MARGIN = 10.0   # filler time = MARGIN x the longest idle host time of a writer


# ---- inputs, made once on the CPU ---------------------------------------------------------------------------------------
def _gridmap(L):
    gm = GridMap(ROWS, COLS, RES, *POS)
    for name in ("elevation", "elevation_masked", "normal_x", "normal_y", "normal_z", "plane_fit_std_dev", "cum_prob"):
        gm.add(name, L[name])
    gm.layers["cum_prob_rowwise"] = np.ascontiguousarray(L["cum_prob_rowwise"], np.float32)
    return gm


def density_vertices(n=3000, seed=5):
    """Roadmap vertices crowded into one corner of the map: the inverse-density term moves the CDF everywhere."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 7))
    v[:, 6] = 1.0
    v[:, 0] = POS[0] + rng.uniform(0.0, 0.5, n) * GEOM[0]
    v[:, 1] = POS[1] + rng.uniform(0.0, 0.5, n) * GEOM[1]
    return v


_INPUTS = {}


def sampler_inputs():
    """The 97 x 61 map of the preprocessing sweep, restated on the CPU (bit-equal to the device's layers:
    test_preprocess_sweep.py), without and with the density term of density_vertices()."""
    if "sampler" not in _INPUTS:
        elev, trav = P.sweep_map(ROWS, COLS, RES, seed=11)
        verts = density_vertices()
        old = _gridmap(P.preprocess(elev, *GEOM, traversability=trav))
        new = _gridmap(P.preprocess(elev, *GEOM, traversability=trav, vertices=verts))
        assert not np.array_equal(old["cum_prob"], new["cum_prob"], equal_nan=True)
        for k in ("elevation", "elevation_masked", "normal_x", "normal_y", "normal_z", "plane_fit_std_dev"):
            assert np.array_equal(old[k], new[k], equal_nan=True), k      # only the CDF changes
        _INPUTS["sampler"] = dict(elev=elev, trav=trav, verts=verts, old=old, new=new)
    return _INPUTS["sampler"]


BLOCK = (28, 16, 40, 30)   # row0, col0, nrows, ncols: 1200 cells, under a quarter of the map (the rectangle path of install)


def _pick_states(gm_old, gm_new, seed):
    """N states of which at least a tenth change their label between the two maps, by the CPU oracle."""
    rob = O.robot("yaml")
    cand = common.random_states(gm_old, 4 * N, np.random.default_rng(seed), z_off=(0.0, 0.01), tilt=0.05, spread=0.4)
    lo = common.oracle_states_valid_threaded(gm_old, rob, cand)
    ln = common.oracle_states_valid_threaded(gm_new, rob, cand)
    diff = np.flatnonzero(lo != ln)[: N // 2]
    same = np.flatnonzero(lo == ln)[: N - len(diff)]
    idx = np.sort(np.concatenate([diff, same]))
    assert len(idx) == N and len(diff) >= N // 10, (len(idx), len(diff))
    return cand[idx], lo[idx], ln[idx]


def rect_inputs():
    """Old map as sampler_inputs(); new map: BLOCK of the body layer raised by 1 m (one update_layer_rects call)."""
    if "rect" not in _INPUTS:
        old = sampler_inputs()["old"]
        new = _gridmap(old.layers)
        e = old["elevation"].copy(order="F")
        r0, c0, nr, nc = BLOCK
        e[r0:r0 + nr, c0:c0 + nc] += np.float32(1.0)
        new.layers["elevation"] = e
        states, lo, ln = _pick_states(old, new, 3)
        _INPUTS["rect"] = dict(old=old, new=new, states=states, labels_old=lo, labels_new=ln)
    return _INPUTS["rect"]


def install_inputs():
    """Old map as sampler_inputs(); new map: the preprocessing of the elevation with BLOCK raised by 1 m."""
    if "install" not in _INPUTS:
        s = sampler_inputs()
        e2 = np.array(s["elev"])
        r0, c0, nr, nc = BLOCK
        e2[r0:r0 + nr, c0:c0 + nc] += np.float32(1.0)
        new = _gridmap(P.preprocess(e2, *GEOM, traversability=s["trav"]))
        states, lo, ln = _pick_states(s["old"], new, 4)
        _INPUTS["install"] = dict(old=s["old"], new=new, elev2=e2, states=states, labels_old=lo, labels_new=ln)
    return _INPUTS["install"]


def cost_inputs():
    if "cost" not in _INPUTS:
        g = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost.npz"))
        crop = g["crop"].astype(np.float32)
        res = float(g["res"])
        other = np.ascontiguousarray(crop[::-1, ::-1].T) * np.float32(0.6) + np.float32(0.05)   # another elevation, same size
        L = crop.shape[0] * res
        rng = np.random.default_rng(9)
        s = rng.uniform(-0.55 * L, 0.55 * L, (N, 2))
        d = rng.uniform(-0.6, 0.6, (N, 2))
        edges = np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, N), s[:, 0], s[:, 1],
                          rng.uniform(-np.pi, np.pi, N)], 1).astype(np.float32)
        _INPUTS["cost"] = dict(crop=crop, other=np.ascontiguousarray(other, np.float32), res=res, L=L, edges=edges,
                               light=mo.random_params(0), full=mo.random_params(0, cw.SHAPES_FULL))
    return _INPUTS["cost"]


# ---- the cases ------------------------------------------------------------------------------------------------------------
class Case:
    """One reader / writer pair on a fresh context holding the OLD state.  read(i) queues the reader on the current lane
    into result i; write() is W; result(i) the host copy; check(old, new, notes) ties the sequential results to the oracle."""
    asynchronous = False      # W returns with its device work queued
    changes_result = True     # old and new results differ (all cases but reachability under a new CDF)

    def __init__(self):
        import torch
        from art_planner_amd.context import Context
        self.torch = torch
        self.ctx = Context(0, "yaml")
        self.keep = []
        self.setup()
        self.ctx.synchronize()
        torch.cuda.synchronize()

    def close(self):
        for k in self.keep:
            if hasattr(k, "close"):
                k.close()
        self.ctx.close()

    def note(self):   # sequential run only, after each read: what check() needs besides the results
        return None

    def result(self, i):
        return self.out[i].cpu().numpy()


class _Sampler(Case):
    def _tensors(self):
        self.out = [self.torch.full((N, 7), -7.0, dtype=self.torch.float64, device=DEV) for _ in range(2)]

    def read(self, i):
        self.ctx.sample_states_dev(17, 100, N, self.out[i])

    def check(self, old, new, notes):
        rob = O.robot("yaml")
        s = sampler_inputs()
        for got, gm in ((old, s["old"]), (new, s["new"])):
            ref, _ = O.OracleSampler(gm).sample(rob, 17, 100, N)
            assert np.abs(got - ref).max() < 1e-12      # test_sampler_matches_oracle's bound


class SampleVsReweight(_Sampler):
    def setup(self):
        s = sampler_inputs()
        self.pm = self.ctx.preprocess_map(s["elev"], *GEOM, traversability=s["trav"])
        self.pm.install()
        self.keep.append(self.pm)
        self.vt = self.torch.tensor(s["verts"], dtype=self.torch.float64, device=DEV)
        self._tensors()

    def write(self):
        self.pm.reweight_dev(self.vt, install_sampler=True)


class SampleVsUpload(_Sampler):
    def setup(self):
        s = sampler_inputs()
        self.ctx.upload_map(s["old"])
        gm = s["new"]
        f = lambda a: np.asfortranarray(a, dtype=np.float32)   # noqa: E731
        self.layers = [f(gm["cum_prob"]), np.ascontiguousarray(gm["cum_prob_rowwise"], np.float32), f(gm["elevation"]),
                       f(gm["normal_x"]), f(gm["normal_y"]), f(gm["normal_z"]), f(gm["plane_fit_std_dev"])]
        self._tensors()

    def write(self):
        gm = sampler_inputs()["new"]
        self.ctx._chk(self.ctx.L.artp_upload_sampler_layers(self.ctx.h, *[a.ctypes.data for a in self.layers], gm.rows,
                                                            gm.cols, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y),
                      "artp_upload_sampler_layers")


class ReachVsReweight(SampleVsReweight):
    """The whole 97 x 61 map (5917 words: no rectangle of it has 4096 cells).  The reweight changes the CDF only, so R and
    R' are both the unchanged labels; a torn read of the packed cells would change them."""
    changes_result = False
    N_YAW = 7

    def _tensors(self):
        self.out = [self.torch.full((ROWS * COLS,), -1, dtype=self.torch.int32, device=DEV) for _ in range(2)]
        self.probe = self.torch.empty((N, 7), dtype=self.torch.float64, device=DEV)

    def read(self, i):
        self.ctx.reachability_map_dev(self.out[i], self.N_YAW)

    def result(self, i):
        return self.out[i].cpu().numpy().view(np.uint32).reshape(COLS, ROWS).T

    def note(self):   # the distribution the sampler draws from at this point
        self.ctx.sample_states_dev(17, 100, N, self.probe)
        self.ctx.synchronize()
        return self.probe.cpu().numpy()

    def check(self, old, new, notes):
        from test_reachability import cells_finite, lattice_poses, mask_bits
        assert np.array_equal(old, new)                     # only the CDF changed
        assert (notes[0] != notes[1]).mean() >= 0.1         # ... and it did change
        gm = sampler_inputs()["old"]
        fin = cells_finite(gm)
        states = lattice_poses(gm, self.N_YAW)[fin].reshape(-1, 7)
        bits = mask_bits(old, self.N_YAW)[fin].reshape(-1)
        ref = common.oracle_states_valid_threaded(gm, O.robot("yaml"), states)
        assert np.array_equal(bits, ref) and 0 < bits.sum() < bits.size and (old[~fin] == 0).all()


class _Cost(Case):
    first, second = "light", "light"   # the network loaded at setup / the one the new features come from

    def setup(self):
        c = cost_inputs()
        self.ctx.cost_load_weights(cw.to_blob(c[self.first]))
        self.ctx.cost_update_map(c["crop"], c["res"], c["L"], c["L"])
        self.edges = self.torch.tensor(c["edges"], device=DEV)
        self.other = self.torch.tensor(c["other"], device=DEV)
        self.out = [self.torch.full((N, 3), -7.0, dtype=self.torch.float32, device=DEV) for _ in range(2)]

    def read(self, i):
        self.ctx.cost_query_dev(self.edges, self.out[i])

    def note(self):
        return self.ctx.cost_features()

    def check(self, old, new, notes):
        c = cost_inputs()
        for got, feats, net in ((old, notes[0], self.first), (new, notes[1], self.second)):
            ref = mo.fc_costs(c[net], np.transpose(feats, (2, 0, 1)), c["edges"], c["res"], c["L"], c["L"])
            if net == "light":
                assert np.abs(got - ref).max() < 5e-5       # test_gpu_cost_full_map_properties' bound
            else:                                           # test_gpu_full_fc_paths_match_the_oracle_on_the_devices_features'
                assert (np.abs(got - ref) <= 1e-4 + 1e-4 * np.abs(ref)).all()
        # the old features are the reference network's (the committed fixture), within test_motion_cost.py's feature bound
        g = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost.npz"))
        if self.first == "light":
            ref = np.transpose(g["features"], (1, 2, 0))
            err = np.abs(notes[0] - ref)
            assert err.max() < 2e-2 + 4e-3 * np.abs(ref).max() and err.mean() < 3e-3


class CostVsUpdateDev(_Cost):
    asynchronous = True

    def write(self):
        c = cost_inputs()
        self.ctx.cost_update_map_dev(self.other, c["res"], c["L"], c["L"])


class CostVsUpdate(_Cost):
    def write(self):
        c = cost_inputs()
        self.ctx.cost_update_map(c["other"], c["res"], c["L"], c["L"])


class CostVsUpdateLayer(_Cost):
    def write(self):
        c = cost_inputs()
        self.ctx.cost_update_map_layer(np.asfortranarray(c["other"]), c["res"], c["L"], c["L"])


class CostVsOtherNetwork(_Cost):
    second = "full"

    def write(self):
        c = cost_inputs()
        self.ctx.cost_load_weights(cw.to_blob(c["full"]))
        self.ctx.cost_update_map(c["other"], c["res"], c["L"], c["L"])


class _Validate(Case):
    def _states(self, inp):
        self.se3 = self.torch.tensor(inp["states"], dtype=self.torch.float64, device=DEV)
        self.out = [self.torch.full((N,), 7, dtype=self.torch.uint8, device=DEV) for _ in range(2)]

    def read(self, i):
        self.ctx.validate_states_dev(self.se3, self.out[i])

    def check(self, old, new, notes):
        inp = self.inputs()
        assert np.array_equal(old, inp["labels_old"]) and np.array_equal(new, inp["labels_new"])


class ValidateVsRects(_Validate):
    asynchronous = True
    inputs = staticmethod(rect_inputs)

    def setup(self):
        inp = rect_inputs()
        self.ctx.upload_map(inp["old"], sampler=False)
        r0, c0, nr, nc = BLOCK
        self.patch = np.asfortranarray(inp["new"]["elevation"][r0:r0 + nr, c0:c0 + nc])
        self._states(inp)

    def write(self):
        self.ctx.update_layer_rects(0, [self.patch], [BLOCK[:2]])


class ValidateVsInstall(_Validate):
    inputs = staticmethod(install_inputs)   # see the module docstring: this writer waits for the other lanes on the host

    def setup(self):
        inp = install_inputs()
        s = sampler_inputs()
        pm = self.ctx.preprocess_map(s["elev"], *GEOM, traversability=s["trav"])
        pm.install()
        self.pm2 = self.ctx.preprocess_map(inp["elev2"], *GEOM, traversability=s["trav"])
        self.keep += [pm, self.pm2]
        self._states(inp)

    def write(self):
        self.pm2.install()


CASES = {
    "sample_states-reweight": SampleVsReweight,
    "sample_states-upload_sampler_layers": SampleVsUpload,
    "reachability_map-reweight": ReachVsReweight,
    "cost_query-cost_update_map_dev": CostVsUpdateDev,
    "cost_query-cost_update_map": CostVsUpdate,
    "cost_query-cost_update_map_layer": CostVsUpdateLayer,
    "cost_query-load_weights-cost_update_map": CostVsOtherNetwork,
    "validate_states-update_layer_rects": ValidateVsRects,
    "validate_states-install": ValidateVsInstall,
}


# ---- the two runs ---------------------------------------------------------------------------------------------------------
def run_case(name, busy=None, fill_seconds=0.0):
    """busy=None: the sequential run (a host wait after every call).  Returns a dict: old, new (R and R'), host_seconds of
    W, busy_before / busy_after (lane 1's stream around W), filler_ok, notes, case (the caller closes it)."""
    import torch
    case = CASES[name]()
    ctx = case.ctx
    sequential = busy is None
    # both lanes on torch streams; in the ordered run lane 1's is one the device runs side by side with lane 0's
    s0 = torch.cuda.Stream(device=DEV)
    s1 = torch.cuda.Stream(device=DEV) if sequential else busy.concurrent_stream(s0)
    if s1 is None:
        case.close()
        raise AssertionError("no stream found whose work overlaps lane 0's: the case would prove nothing")
    with torch.cuda.stream(s0):
        ctx.use_torch_stream()
    ctx.set_lane(1)
    with torch.cuda.stream(s1):
        ctx.use_torch_stream()
    ctx.set_lane(0)
    ctx.synchronize()
    notes = []
    if not sequential:
        busy.queue(s1, fill_seconds)
    ctx.set_lane(1)
    case.read(0)
    if sequential:
        ctx.synchronize()
        notes.append(case.note())
    ctx.set_lane(0)
    busy_before = not s1.query()
    t0 = time.perf_counter()
    case.write()
    host = time.perf_counter() - t0
    busy_after = not s1.query()
    if sequential:
        ctx.synchronize()
    ctx.set_lane(1)
    case.read(1)
    ctx.set_lane(0)
    ctx.synchronize()
    torch.cuda.synchronize()
    if sequential:
        ctx.set_lane(1)
        notes.append(case.note())
        ctx.set_lane(0)
    out = dict(old=case.result(0), new=case.result(1), host_seconds=host, busy_before=busy_before, busy_after=busy_after,
               filler_ok=sequential or busy.result_is_expected(), notes=notes, case=case)
    return out


@pytest.fixture(scope="module")
def sequential():
    """Every case run sequentially, once: name -> (old, new, idle host time of W); the oracle checks happen here."""
    seq = {}

    def get(name):
        if name not in seq:
            r = run_case(name)
            try:
                r["case"].check(r["old"], r["new"], r["notes"])
                if r["case"].changes_result:
                    frac = float((r["old"] != r["new"]).mean())
                    assert frac >= 0.1, f"{name}: old and new results differ in {frac:.3f} of their elements"
            finally:
                r["case"].close()
            seq[name] = (r["old"], r["new"], r["host_seconds"])
        return seq[name]

    for name in CASES:   # all of them: the filler is sized by the slowest writer
        get(name)
    return seq


@pytest.fixture(scope="module")
def busy():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return Busy(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_shared_state_write_is_ordered_against_a_lane_in_flight(name, sequential, busy):
    old, new, _ = sequential[name]
    fill = min(CEILING_S, MARGIN * max(t for _, _, t in sequential.values()))
    r = run_case(name, busy, fill)
    case = r["case"]
    try:
        print(f"{name}: filler {fill * 1e3:.1f} ms ({busy.repeats(fill)} products of {busy.seconds_per_product * 1e3:.3f} ms), "
              f"W host {r['host_seconds'] * 1e3:.3f} ms, busy before / after W: {r['busy_before']} / {r['busy_after']}, "
              f"R == old: {np.array_equal(r['old'], old)}, R' == new: {np.array_equal(r['new'], new)}")
        assert r["busy_before"], "lane 1's stream had drained before W was called: the case proves nothing"
        if case.asynchronous:
            assert r["busy_after"], "lane 1's stream had drained when W returned: the case proves nothing"
        assert r["filler_ok"]
        assert np.array_equal(r["old"], old), "W overtook the reader queued on lane 1"
        assert np.array_equal(r["new"], new), "the reader queued on lane 1 after W ran ahead of it"
    finally:
        case.close()
