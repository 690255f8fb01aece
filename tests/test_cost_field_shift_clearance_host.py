"""Planner::shiftClearanceCostField through the C++ host mirror (art_planner_amd/host/test_cost_field_shift_clearance_clearance.cpp):
a kept clearance-weighted field carried onto a map moved by (6, -4) cells, and back, equals a second
computeClearanceCostField on that map bit for bit; the planner's "cost_to_go" layer follows; the refusals throw and leave
the field as it was."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_shift_clearance")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_shift_clearance"])
    assert os.path.exists(BIN)


def test_cost_field_shift_clearance_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_shift_clearance_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 + 0 mismatches" in r.stdout, r.stdout
