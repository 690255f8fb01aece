"""Planner::updateClearanceCostField through the C++ host mirror (art_planner_amd/host/test_cost_field_clearance_update.cpp):
a kept clearance-weighted field, updated after a mask edit and after an edit with refreshed heights, equals a new
computeClearanceCostField bit for bit each time, and the planner's map carries the updated "cost_to_go"."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_clearance_update")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_clearance_update"])
    assert os.path.exists(BIN)


def test_cost_field_clearance_update_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_clearance_update_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 layer cells stale, 0 differ from a new field" in r.stdout, r.stdout
