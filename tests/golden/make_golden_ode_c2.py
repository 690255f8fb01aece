#!/usr/bin/env python3
"""The real patched ODE (oracle/_ref, compiled from /root/reference/ode where it lies) on the benchmark's C2 map:
20 000 torso and 60 000 foot dPoses of the YAML robot around the 400 x 400 @ 0.04 m Perlin terrain of
synthetic.make_map(400, 0.04, seed=1234).

Build container only.  Writes tests/golden/ode_c2.npz: the map's elevation layer and the mask of elevation_masked
(the map is built with sin / cos, not bit-reproducible across CPUs), per case the seed and sha1 of the poses
(tests/golden_io.py regenerates them) and the reference's hit bits.  The oracle must agree everywhere."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_io as G  # noqa: E402
import oracle_py as O  # noqa: E402
from synthetic import make_map  # noqa: E402


def main():
    assert O.have_ref(), "build the reference first: make -C oracle ref"
    gm = make_map(400, 0.04, seed=1234)
    elev = np.asarray(gm["elevation"], np.float32)
    em = np.asarray(gm["elevation_masked"], np.float32)
    mask = em != elev
    assert np.isneginf(em[mask]).all(), "elevation_masked is elevation with -inf where masked"
    out = {"elevation": elev, "masked": np.packbits(mask.ravel()), "res": np.float64(gm.res),
           "pos_x": np.float64(gm.pos_x), "pos_y": np.float64(gm.pos_y)}
    rob = O.robot("yaml")
    for ci, (part, layer, zoff, n) in enumerate(G.ODE_C2_CASES):
        seed = 940000 + ci
        P = G.bulk_pose_params(gm, n, seed, zoff, tilt=G.ODE_C2_TILT)
        side = getattr(rob, part)
        ref = O.RefChecker(side, gm[layer], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
        hit = ref.check(P)
        ref.close()
        hit_o = O.OracleField(gm[layer], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y).check_boxes(side, P)
        assert np.array_equal(hit, hit_o), (part, int((hit != hit_o).sum()))
        out[f"{part}__seed"] = np.int64(seed)
        out[f"{part}__sha1"] = np.array(G.sha1_of(P))
        out[f"{part}__hit"] = np.packbits(hit)
        print(f"{part:6s} n={n} hit={hit.mean():.3f}")
    np.savez_compressed(os.path.join(HERE, "ode_c2.npz"), **out)


if __name__ == "__main__":
    main()
