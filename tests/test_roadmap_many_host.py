"""artp_roadmap_solve_many through the C ABI without a device (exported, refuses bad arguments) and through the C++
host mirror (art_planner_amd/host: BatchPRM::solveMany, test_roadmap_many.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from art_planner_amd import _capi

HOST = os.path.join(common.ROOT, "art_planner_amd", "host")
BIN = os.path.join(HOST, "test_roadmap_many")


def _build():
    subprocess.check_call(["make", "-s", "-C", HOST])
    assert os.path.exists(BIN)


def test_solve_many_is_exported_and_refuses_bad_arguments():
    L = _capi.load()
    assert hasattr(L, "artp_roadmap_solve_many")
    s = np.zeros(7)
    st = np.zeros(4, np.int32)
    cost = np.zeros(4)
    # no handle
    assert L.artp_roadmap_solve_many(None, s.ctypes.data, s.ctypes.data, 1, st.ctypes.data, cost.ctypes.data,
                                     None, None, 0, None) == -1
    assert L.artp_roadmap_solve_many(None, None, None, 0, None, None, None, None, 0, None) == -1
    # goals NULL with n_goals > 0 (the handle is never dereferenced before the argument check)
    fake = C.c_void_p(1)
    assert L.artp_roadmap_solve_many(fake, s.ctypes.data, None, 3, st.ctypes.data, cost.ctypes.data,
                                     None, None, 0, None) == -1


def test_roadmap_many_host_test_builds():
    """Builds with `make all`; without a device the constructor throws (exit 3, no CPU fallback)."""
    _build()
    import torch
    if torch.cuda.is_available():
        return
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_roadmap_many_host_test_on_the_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal to the sequential queries" in r.stdout, r.stdout
