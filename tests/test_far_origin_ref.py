"""CPU checks of the far-origin inputs (tests/far_origin.py): the conditions that keep tests/test_far_origin.py (-m gpu)
from being vacuous.  At every origin the state list mixes valid and invalid states, its boxes leave the checker through
every exit the fast paths decide, the edge list mixes accepted and refused motions; at the two farthest origins the
oracle's own labels and the restated normals really depend on the origin (a kernel that is only right in the frame of
origin zero cannot pass there); and the float64 bounds of the preprocessing hold at all but the UTM origin, where the
normal bound's cap of 1e-5 is below the rounding of a cell centre."""
import numpy as np
import pytest

import far_origin as FO
import oracle_py as O
from test_preprocess_sweep import POS, _expected, _float64_violations

ORIGINS = list(FO.ORIGINS)
MAPS = list(FO.MAPS)
PRE_POINTS = ("odd97x61", "res0.1", "defaults-robot")
TORSO_CODES = (1, 5, 6, 8)
FOOT_CODES = (0, 1, 2, 3, 5, 6, 8)


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_validity_mix(name, origin):
    lab = FO.oracle_labels(name, FO.ORIGINS[origin])
    assert len(lab) == 20000
    print(f"{name}/{origin}: valid share {lab.mean():.4f}")
    assert 0.03 <= lab.mean() <= 0.97


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_exit_codes_of_the_states_boxes(name, origin):
    pos = FO.ORIGINS[origin]
    rob = O.robot(FO.ROBOT)
    om = O.OracleMap(FO.map_at(name, pos))
    torso, feet = FO.state_boxes(name, pos)
    assert len(torso) == 5000 and len(feet) == 20000
    _, et, _ = om.body.check_boxes(rob.torso, torso, want_detail=True)
    _, ef, _ = om.feet.check_boxes(rob.foot, feet, want_detail=True)
    ct = {c: int((et == c).sum()) for c in TORSO_CODES}
    cf = {c: int((ef == c).sum()) for c in FOOT_CODES}
    print(f"{name}/{origin}: torso {ct} foot {cf}")
    assert min(ct.values()) >= 100, ct
    assert min(cf.values()) >= 100, cf


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_edge_mix(name, origin):
    pos = FO.ORIGINS[origin]
    a, b = FO.edge_pairs(name, pos)
    assert len(a) >= 1500
    assert (np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]) < 1.5).all()
    ref = FO.oracle_edges(name, pos)
    print(f"{name}/{origin}: {len(a)} pairs, checkMotion accepts {ref['ok'].mean():.3f}, 0.5 m rule {ref['ei'].mean():.3f}")
    assert 0.10 <= ref["ok"].mean() <= 0.90
    assert np.array_equal(ref["ok"], ref["lv_ok"])
    assert (ref["lv_t"][ref["ok"] == 0] < 1.0).all()


@pytest.mark.parametrize("origin", ["far", "utm"])
@pytest.mark.parametrize("name", MAPS)
def test_labels_depend_on_the_origin(name, origin):
    """The same cells and perturbations (the sampler's (seed, index) picks them whatever the position) get other labels
    at the far origins: the float rounding of a world coordinate decides them there."""
    pos = FO.ORIGINS[origin]
    assert np.array_equal(FO.states(name, pos)[:, 2:], FO.states(name, FO.ZERO)[:, 2:])
    differ = int((FO.oracle_labels(name, pos) != FO.oracle_labels(name, FO.ZERO)).sum())
    print(f"{name}/{origin}: {differ} of 20000 oracle labels differ from origin zero")
    assert differ >= 1


@pytest.mark.parametrize("origin", ["far", "utm"])
def test_random_states_moved_with_the_map_change_labels(origin):
    """The same holds with common.random_states moved with the map."""
    name, pos = "p160", FO.ORIGINS[origin]
    rob = O.robot(FO.ROBOT)
    l0 = O.OracleMap(FO.base_map(name)).states_valid(rob, FO.random_moved_states(name, FO.ZERO))
    l1 = O.OracleMap(FO.map_at(name, pos)).states_valid(rob, FO.random_moved_states(name, pos))
    print(f"{name}/{origin}: {int((l0 != l1).sum())} of {len(l0)} labels of moved random states differ from origin zero")
    assert (l0 != l1).any()


@pytest.mark.parametrize("point", PRE_POINTS)
def test_normals_depend_on_the_origin(point):
    near = _expected(point, POS)[-1]
    zeros_near = int(((near["normal_x"] == 0) & (near["normal_y"] == 0) & (near["normal_z"] == 0)).sum())
    for origin in ("far", "utm"):
        L = _expected(point, FO.ORIGINS[origin])[-1]
        d = max(float(np.abs(L[k] - near[k]).max()) for k in ("normal_x", "normal_y", "normal_z"))
        zeros = int(((L["normal_x"] == 0) & (L["normal_y"] == 0) & (L["normal_z"] == 0)).sum())
        print(f"{point}/{origin}: largest |normal - normal at {POS}| {d:.3e}; all-zero normals {zeros} (near: {zeros_near})")
        assert d > 0


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("point", PRE_POINTS)
def test_float64_bounds_hold_at_all_but_the_utm_origin(point, origin):
    """The restatement itself against its float64 reference: inside the bounds at "odom", "km" and "far"; at "utm" a cell
    centre is rounded by up to 0.25 m and the normal bound, capped at 1e-5, cannot hold -- which is why the device test
    applies the bounds at the first three only."""
    pt, prm, rob, geom, (elev, trav, obs, verts), L = _expected(point, FO.ORIGINS[origin])
    bad = _float64_violations(L, L, elev, geom, prm, rob)
    if origin == "utm":
        assert any(b.startswith("float64:normal") for b in bad), bad
    else:
        assert not bad, bad
