"""Planner::computeCostFields and Planner::computeCostMatrix through the C++ host mirror
(art_planner_amd/host/test_cost_field_many.cpp): four source sets in one batched call equal Planner::computeCostField on
each set bit for bit (dist, reached_nodes, the path to the farthest node); the matrix of five poses equals those fields'
dist at the poses, in one group and in groups of two; the fields outlive one another; a bad source throws and names its set."""
import os
import subprocess

import pytest

import common

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_cost_field_many")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST, "test_cost_field_many"])
    assert os.path.exists(BIN)


def test_cost_field_many_host_test_builds():
    """Builds with the host Makefile; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_cost_field_many_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cost fields: 0 mismatches" in r.stdout, r.stdout
    assert "cost matrix: 0 mismatches" in r.stdout, r.stdout
