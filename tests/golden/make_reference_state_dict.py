#!/usr/bin/env python3
"""Build container only: the layout of the REFERENCE network's state_dict
(art_planner_motion_cost/.../predictor/network_light.py, imported where it lies) -- the file format
predictor.py:20 torch.load()s (`self.network.load_state_dict(torch.load(modelFile))`).

Writes tests/golden/reference_state_dict.json: every entry of network_light.network().state_dict() in the
class's own order with its shape and dtype (and the value of the BatchNorm num_batches_tracked counters), after
loading the seeded parameters of tools/convert_weights.random_params(0) into the class.  Data only, no reference
source text.  tests/test_motion_cost.py rebuilds that checkpoint from the manifest and the seeded parameters, so
tools/convert_weights.py main() is exercised on a real torch-saved checkpoint of the reference's layout (the
repository's trained checkpoints are git-LFS stubs).  Usage: make_reference_state_dict.py [out.json]"""
import json
import os
import sys

import torch

sys.dont_write_bytecode = True  # the reference tree is read-only: no __pycache__ next to its sources
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = "/root/reference/art_planner_motion_cost/src/art_planner_motion_cost/predictor"


def build_state_dict(seed=0):
    sys.path.insert(0, REF)
    import network_light  # the reference
    import convert_weights
    params = convert_weights.random_params(seed)
    net = network_light.network().eval()
    sd = net.state_dict()
    missing = [k for k in sd if not k.endswith("num_batches_tracked") and k not in params]
    assert not missing, missing
    for k in sd:
        if not k.endswith("num_batches_tracked"):
            assert tuple(sd[k].shape) == params[k].shape, (k, sd[k].shape, params[k].shape)
            sd[k] = torch.from_numpy(params[k].copy())
    net.load_state_dict(sd)
    return net.state_dict()


def manifest(sd):
    out = []
    for k, v in sd.items():
        e = {"key": k, "shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
        if k.endswith("num_batches_tracked"):
            e["value"] = int(v.item())
        out.append(e)
    return {"what": "network_light.network().state_dict() of the reference, seeded parameters random_params(0) "
                    "loaded: entries in the class's order (tests/golden/make_reference_state_dict.py)",
            "entries": out}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "reference_state_dict.json")
    with open(path, "w") as f:
        json.dump(manifest(build_state_dict(0)), f, indent=1)
        f.write("\n")
