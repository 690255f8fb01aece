"""CPU checks of the robot geometries (tests/robot_geometry.py): the conditions that keep tests/test_robot_geometry.py
(-m gpu) from being vacuous, and artp_create's refusal of parameters no kernel may see.

For every geometry on both maps the state list mixes valid and invalid states, its boxes leave the checker through at
least four exits, the edge list mixes accepted and refused motions under each of the three rules, and the upload is
accepted by the restated size_scratch.  Over the table the box windows reach the table tiers written down here; and the
torso offset decides labels term by term, so a kernel that drops, swaps or mis-signs one cannot be bit-equal."""
import ctypes as C
import math

import numpy as np
import pytest

import common
import oracle_py as O
import robot_geometry as RG

GEOS = list(RG.GEOMETRIES)
MAPS = list(RG.MAPS)
ARTP_ERR_INVALID_ARG, ARTP_ERR_NO_DEVICE = -1, -2


@pytest.mark.parametrize("mname", MAPS)
@pytest.mark.parametrize("name", GEOS)
def test_validity_mix(name, mname):
    lab = RG.oracle_labels(name, mname)
    assert len(lab) == RG.N_STATES
    print(f"{name}/{mname}: valid share {lab.mean():.4f}")
    assert 0.05 <= lab.mean() <= 0.95


@pytest.mark.parametrize("mname", MAPS)
@pytest.mark.parametrize("name", GEOS)
def test_exit_codes(name, mname):
    """At least four exits with ten or more boxes each, for the torso and for the feet: among the states' own boxes given
    to check_boxes, and among the details validate_states reports (codes below 1 there: a box outside the map or not
    looked at)."""
    rob = RG.robot_of(name)
    om = O.OracleMap(RG.map_of(mname))
    torso, feet = RG.state_boxes(name, mname)
    assert len(torso) == RG.N_BOXES and len(feet) == RG.N_BOXES
    _, et, _ = om.body.check_boxes(rob.torso, torso, want_detail=True)
    _, ef, _ = om.feet.check_boxes(rob.foot, feet, want_detail=True)
    det = RG.oracle_details(name, mname)
    for what, codes in (("torso boxes", et), ("foot boxes", ef), ("torso details", det[:, 0][det[:, 0] > 0]),
                        ("foot details", det[:, 1:5][det[:, 1:5] > 0])):
        cnt = {int(c): int((codes == c).sum()) for c in np.unique(codes)}
        print(f"{name}/{mname}: {what} {cnt}")
        assert sum(v >= 10 for v in cnt.values()) >= 4, (what, cnt)


@pytest.mark.parametrize("mname", MAPS)
@pytest.mark.parametrize("name", GEOS)
def test_edge_mix(name, mname):
    a, b = RG.edge_pairs(name, mname)
    assert len(a) >= 1000
    assert (np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]) < RG.PAIR_DIST_OF.get(name, RG.PAIR_DIST)).all()
    ref = RG.oracle_edges(name, mname)
    print(f"{name}/{mname}: {len(a)} pairs, checkMotion {ref['ok'].mean():.3f}, lastValid {ref['lv_ok'].mean():.3f}, "
          f"0.5 m rule {ref['ei'].mean():.3f}")
    for rule in ("ok", "lv_ok", "ei"):
        assert 0.05 <= ref[rule].mean() <= 0.95, rule
    assert (ref["lv_t"][ref["lv_ok"] == 0] < 1.0).all()


@pytest.mark.parametrize("mname", MAPS)
@pytest.mark.parametrize("name", GEOS)
def test_sizing_accepts(name, mname):
    n, res, _ = RG.MAPS[mname]
    sz = RG.sizing(RG.robot_of(name), n, res)
    print(f"{name}/{mname}: {sz}")
    assert sz["accepted"]
    assert 4 <= sz["foot_tile"] <= sz["tile"] <= 64 and min(sz["partner_radius"]) > 0


def test_sizing_restates_the_window_tile_and_refuses_what_the_library_refuses():
    """The tile is the one tests/test_resolution_sweep.py restates, for the presets and the table; one step past the
    finest accepted spacing is refused."""
    from test_resolution_sweep import _maxdim, finest_accepted
    for rob in [O.robot("yaml"), O.robot("defaults")] + [RG.robot_of(g) for g in GEOS]:
        for n, res in ((120, 0.05), (60, 0.1), (320, 0.03)):
            assert RG.sizing(rob, n, res)["tile"] == max(_maxdim(rob, n, res), 4)
    for kind in ("yaml", "defaults"):
        n, res, n2, res2 = finest_accepted(O.robot(kind))
        assert RG.sizing(O.robot(kind), n, res)["accepted"] and not RG.sizing(O.robot(kind), n2, res2)["accepted"]


def test_sizing_extremes_of_the_table():
    """What the table is there for: the largest torso tile (tall, fine), the foot that sizes the tile and fills the feet's
    1024-triangle list, and a few-state LDS above the 64 KiB that need the opt-in (bigfeet, fine)."""
    n, res, _ = RG.MAPS["fine"]
    assert RG.sizing(RG.robot_of("tall"), n, res)["tile"] == 40
    sz = RG.sizing(RG.robot_of("bigfeet"), n, res)
    assert sz["foot_tile"] == sz["tile"] == 25 and sz["foot_list"] == 1024 and 2 * 24 * 24 > 1024
    assert 64 * 1024 < sz["lds"]["few"] <= 160 * 1024
    assert max(RG.sizing(RG.robot_of(g), n, res)["lds"]["few"] for g in GEOS) == sz["lds"]["few"]
    coarse = RG.sizing(RG.robot_of("bigfeet"), *RG.MAPS["coarse"][:2])
    assert coarse["lds"]["few"] < 64 * 1024        # the second upload on one context sizes the LDS downwards


# the union over the table and both maps (window_classes: an estimate from the oracle's box poses)
REACHED = {
    ("torso", "coarse"): {"<=7", "<=13", "<=25", ">25"},
    ("foot", "coarse"): {"<=7", "<=13", "<=25"},
    ("torso", "stats"): {"<8", "<16", "<32", ">=32"},
    ("foot", "stats"): {"<4", "<8", "<16", "<32"},
}


def test_window_classes_reached_over_the_table():
    got = {k: set() for k in REACHED}
    hist = {}
    for name in GEOS:
        for mname in MAPS:
            wc = RG.window_classes(RG.robot_of(name), RG.map_of(mname), RG.states(name, mname))
            hist[(name, mname)] = wc
            print(f"{name}/{mname}: {wc}")
            for (kind, tier) in REACHED:
                got[(kind, tier)] |= set(wc[kind][tier])
    assert got == REACHED
    # the windows the presets' aspect ratios never give
    f = hist[("bigfeet", "fine")]["foot"]
    assert f["sides"][0] >= 13 and f["sides"][1] >= 20 and set(f["coarse"]) == {"<=25"}     # large foot, small torso
    assert hist[("bigfeet", "fine")]["torso"]["sides"][1] < f["sides"][1]
    assert hist[("plank", "fine")]["foot"]["sides"] == (4, 13)                                # thin and long
    assert "<4" in hist[("tiny", "fine")]["foot"]["stats"] and "<4" in hist[("plank", "coarse")]["foot"]["stats"]
    assert ">=32" in hist[("tall", "fine")]["torso"]["stats"]


def test_the_torso_offset_decides_labels():
    """On one list of 20 000 states on the fine map: the offset against none, each of its two planar terms alone, and
    the two exchanged."""
    gm = RG.map_of("fine")
    se3 = RG.sample_states(gm, RG.robot_of("yaml"), 20000)
    o = RG.GEOMETRIES["offset"]

    def labels(**over):
        rob = O.robot("yaml")
        for k, v in over.items():
            setattr(rob, k, v)
        return common.oracle_states_valid_threaded(gm, rob, se3)

    none, full = labels(), labels(**o)
    swapped = labels(**dict(o, torso_off_x=o["torso_off_y"], torso_off_y=o["torso_off_x"]))
    counts = dict(offset=int((full != none).sum()), x_alone=int((labels(torso_off_x=o["torso_off_x"]) != none).sum()),
                  y_alone=int((labels(torso_off_y=o["torso_off_y"]) != none).sum()),
                  exchanged=int((swapped != full).sum()))
    print(counts)
    assert min(counts.values()) > 0, counts


def test_params_and_robot_are_filled_from_one_table():
    for name in GEOS:
        prm, rob = RG.params_of(name), RG.robot_of(name)
        for f, _ in O.Robot._fields_:
            assert getattr(prm, f) == getattr(rob, f), (name, f)
        for k, v in RG.GEOMETRIES[name].items():
            assert getattr(rob, k) == v


def test_halo_restatement_follows_the_offset():
    from test_reachability import halo_cells
    y, o = RG.robot_of("yaml"), RG.robot_of("offset")
    assert halo_cells(o, 0.05) > halo_cells(y, 0.05) > 4
    b = RG.robot_of("bigfeet")          # the feet decide: |(0.5, 0.5)| + half of |(0.7, 0.7, 0.3)|
    assert halo_cells(b, 0.05) == math.ceil((math.hypot(0.5, 0.5) + 0.5 * math.sqrt(0.49 + 0.49 + 0.09)) / 0.05) + 4


def test_preprocessing_sizes_of_the_three_geometries():
    """What the preprocessing reads of a robot (tests/preprocess_restated.py): reach and wall footprints, normal terms, blur
    taps.  tiny: footprints of 0 cells at 0.1 m and 1 at 0.05 m; bigfeet: min_wall < 0, and the restatement takes the
    3 x 3 rectangle for every size <= 0 (cv::erode / cv::dilate with an empty kernel, oracle/map_processors._disk)."""
    import preprocess_restated as P
    got = {(g, res): P.reach_sizes(RG.robot_of(g), res) for g in ("tiny", "bigfeet", "wide") for res in (0.1, 0.05)}
    print(got)
    assert got[("tiny", 0.1)] == (0, 0) and got[("tiny", 0.05)] == (1, 1)
    assert got[("bigfeet", 0.1)] == (9, -1) and got[("bigfeet", 0.05)] == (19, -2)
    assert min(got[("wide", 0.1)]) >= 2
    for size in (0, -1, -2):
        assert P.disk(size).shape == (3, 3) and P.disk(size).all()
    m = np.ones((7, 9), np.float32)
    m[3, 4] = 0.0
    assert (P.erode(m, -1) == 0).sum() == 9 and (P.dilate(1 - m, 0) == 1).sum() == 9
    # normal terms and blur taps differ from the presets'
    assert P.normal_counts(RG.robot_of("tiny"), 0.1) == (1, 0) and P.normal_counts(O.robot("yaml"), 0.1) == (4, 3)
    assert P.gauss_taps(RG.robot_of("tiny"), 0.1)[0] == 7 and P.gauss_taps(RG.robot_of("wide"), 0.05)[0] == 53


# ---- artp_create refuses what no kernel may see -----------------------------------------------------------------------------
SIZES = ("torso_length", "torso_width", "torso_height", "reach_x", "reach_y", "reach_z")
OFFSETS = ("torso_off_x", "torso_off_y", "torso_off_z", "feet_off_x", "feet_off_y", "feet_off_z")
LIMITS = ("max_pitch_pert", "max_roll_pert")
NOT_FINITE = (float("nan"), float("inf"), -float("inf"))
BAD = ([(f, v) for f in SIZES for v in NOT_FINITE + (0.0, -0.0, -0.3)] + [(f, v) for f in OFFSETS for v in NOT_FINITE] +
       [(f, v) for f in LIMITS for v in NOT_FINITE + (-1e-9,)])


def _create(prm):
    from art_planner_amd import _capi
    L = _capi.load()
    h = C.c_void_p(0xdead)               # not NULL going in
    rc = L.artp_create(0, C.byref(prm), C.byref(h))
    return L, rc, h


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_artp_create_refuses_one_bad_field(field, value):
    from art_planner_amd.context import make_params
    prm = make_params("yaml")
    setattr(prm, field, value)
    _, rc, h = _create(prm)
    assert rc == ARTP_ERR_INVALID_ARG
    assert h.value is None                # *out == NULL


@pytest.mark.parametrize("name", ["yaml-preset", "defaults-preset"] + GEOS)
def test_artp_create_lets_usable_parameters_past_the_check(name):
    """The presets unmodified and every geometry of the table (zero limits and negative offsets among them): 0 with a
    device, ARTP_ERR_NO_DEVICE without one -- never the refusal."""
    from art_planner_amd.context import make_params
    prm = make_params(name.split("-")[0]) if name.endswith("-preset") else RG.params_of(name)
    L, rc, h = _create(prm)
    assert rc in (0, ARTP_ERR_NO_DEVICE), rc
    if rc == 0:
        assert h.value
        L.artp_destroy(h)
    else:
        assert h.value is None
