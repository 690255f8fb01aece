"""Planner::blockCostFieldMoves, unblockCostField and planOnCostField through the C++ host mirror
(art_planner_amd/host/test_cost_field_plan.cpp): a kept field with a blocked move equals a second field with the same move
blocked bit for bit and gives the first field back when unblocked; every move of a planned path passes artp_check_motions,
and the field the plan leaves equals a second field with the same set blocked in one call."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_plan")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_plan"])
    assert os.path.exists(BIN)


def test_cost_field_plan_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_plan_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 + 0 mismatches" in r.stdout, r.stdout
