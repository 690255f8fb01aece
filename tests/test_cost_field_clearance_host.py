"""Planner::computeClearance and computeClearanceCostField through the C++ host mirror
(art_planner_amd/host/test_cost_field_clearance.cpp): the facade's clearance map equals a brute-force loop over the
definition, a clearance field with gain 0 equals computeCostField's bit for bit, and every move of a path planned on a kept
clearance field passes artp_check_motions."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_clearance")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_clearance"])
    assert os.path.exists(BIN)


def test_cost_field_clearance_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_clearance_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout, r.stdout
