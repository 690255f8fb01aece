"""Planner::updateLearnedCostField through the C++ host mirror (art_planner_amd/host/test_cost_field_learned_update.cpp):
a kept learned field, updated after the cost map, the mask and both changed, equals a new computeLearnedCostField bit for
bit each time, and the planner's map carries the updated "cost_to_go"."""
import os
import subprocess
import sys

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_learned_update")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_learned_update"])
    assert os.path.exists(BIN)


def test_cost_field_learned_update_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_learned_update_host_test_on_the_gpu(tmp_path):
    _build()
    sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import convert_weights as cw
    import cost_exact_ref as R
    import motion_cost_oracle as mo
    blob = tmp_path / "weights.blob"
    blob.write_bytes(cw.to_blob(mo.random_params(0, R.shapes_of(1))))   # the seeded parameters of the cost tests
    r = subprocess.run([BIN, str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 layer cells stale, 0 differ from a new field" in r.stdout, r.stdout
