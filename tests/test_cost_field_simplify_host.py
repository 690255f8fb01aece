"""Planner::simplifyCostFieldPaths and planOnCostField(simplify = true) through the C++ host mirror
(art_planner_amd/host/test_cost_field_simplify.cpp): checked lattice paths simplified with a covering window equal
artp_roadmap_simplify_path bit for bit; with window 16 every kept pair passes artp_check_motions and
artp_check_edges_interp, and planOnCostField(simplify = true) on a second field holds the same bits."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_simplify")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_simplify"])
    assert os.path.exists(BIN)


def test_cost_field_simplify_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_simplify_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 + 0 mismatches" in r.stdout, r.stdout
