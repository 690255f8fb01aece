"""The tree planner names through the C++ host mirror (art_planner_amd/host: Planner with params.planner.name =
"rrt_star" / "inf_rrt_star" / "rrt_sharp", BatchTree over artp_tree_*), and the C ABI's tree section without a device."""
import ctypes as C
import os
import subprocess

import pytest

import common
from art_planner_amd import _capi

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_tree_planner")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST])
    assert os.path.exists(BIN)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_tree_planner_host_test_builds_and_answers_for_the_device():
    """Builds with `make all`; without a device the constructor throws (exit 3, no CPU fallback), with one it plans."""
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == (0 if _have_gpu() else 3), r.stdout + r.stderr


def test_tree_params_defaults():
    L = _capi.load()
    p = _capi.TreeParams()
    L.artp_tree_params_defaults(C.byref(p))
    assert (p.seed, p.first_index, p.variant, p.objective) == (42, 0, 0, 0)
    assert (p.max_lon_vel, p.max_lat_vel, p.max_ang_vel) == (0.5, 0.1, 0.5)   # params.h:71-73
    assert (p.batch, p.max_vertices, p.max_batches) == (1024, 100000, 0)
    assert (p.plan_time, p.range, p.rewire_factor, p.profile) == (0.0, 0.0, 1.1, 0)
    assert C.sizeof(_capi.TreeParams) == 96


def test_tree_entry_points_refuse_null_handles():
    L = _capi.load()
    n = C.c_size_t(0)
    assert L.artp_tree_grow(None, 1, None) == -1
    assert L.artp_tree_solve(None, None, 0, C.byref(n), None) == -1
    assert L.artp_tree_stats(None, None) == -1
    assert L.artp_tree_export(None, None, None, None, None, None, None) == -1
    assert L.artp_tree_export_checked(None, None, None, None, None, 0, C.byref(n)) == -1
    assert L.artp_tree_create(None, None, None, None, None) == -1
    L.artp_tree_destroy(None)


@pytest.mark.gpu
def test_tree_planner_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("rrt_star", "inf_rrt_star", "rrt_sharp"):
        assert f"{name}: SOLVED" in r.stdout, r.stdout
