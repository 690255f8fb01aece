"""Planner::computeLearnedCostFields / computeClearanceCostFields and the two weighted cost matrices through the C++ host
mirror (art_planner_amd/host/test_cost_field_many_weighted.cpp): under each cost, three source sets in one batched call
equal the single call on each set bit for bit (dist, reached_nodes, the path to the farthest node, the clearance map); the
matrix of four poses equals the single fields' dist at the poses, in one group and in groups of three, on one table; the
fields outlive the one that built the table; a bad source throws and names its set."""
import os
import subprocess
import sys

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_many_weighted")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_many_weighted"])
    assert os.path.exists(BIN)


def test_cost_field_many_weighted_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_many_weighted_host_test_on_the_gpu(tmp_path):
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
    assert "learned fields: 0 mismatches" in r.stdout, r.stdout
    assert "clearance fields: 0 mismatches" in r.stdout, r.stdout
    assert "learned matrix: 0 mismatches" in r.stdout, r.stdout
    assert "clearance matrix: 0 mismatches" in r.stdout, r.stdout
