#!/usr/bin/env python3
"""Golden vectors for the exact k-nearest-pose search over poses of J joints (posendf_amd.knn.PoseIndex(num_joints=J);
include/posendf_amd_skeleton_data.h), produced by the REFERENCE itself: its data/dist_utils.py `dist_calc` (classes `geo` and `euc`,
unweighted: the mean over the joint axis, whatever its length) with every query's candidate list being the whole database, as
tests/golden/make_golden_knn.py does for 21 joints.  The module imports smplx, pytorch3d and ipdb at the top without using them in
these classes: they are stubbed.  Inputs come from tests/skeleton_data_oracle.knn_inputs (seeded), so only the outputs are stored.
usage: python tests/golden/make_golden_skeleton_knn.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from skeleton_data_oracle import knn_inputs  # noqa: E402

for name in ("smplx", "ipdb", "pytorch3d"):
    sys.modules[name] = types.ModuleType(name)
tr = types.ModuleType("pytorch3d.transforms")
for fn in ("axis_angle_to_quaternion", "quaternion_to_axis_angle", "axis_angle_to_matrix"):
    setattr(tr, fn, None)
sys.modules["pytorch3d.transforms"] = tr
sys.path.insert(0, "/root/reference/data")
import dist_utils  # noqa: E402

Q, N, SEED = 16, 2000, 5
JOINTS = (15, 32)


def main():
    out = {"torch_version": np.array(torch.__version__)}
    for J in JOINTS:
        q, db = knn_inputs(Q, N, J, SEED)
        valid = torch.from_numpy(db)[None].expand(Q, N, J, 4)
        for metric in ("geo", "euc"):
            calc = getattr(dist_utils, metric)(Q, device="cpu", weighted=False)
            val, idx = calc.dist_calc(torch.from_numpy(q), valid, N, 5)
            out[f"{metric}_u_{J}_val"] = val.numpy()
            out[f"{metric}_u_{J}_idx"] = idx.numpy()
    np.savez_compressed(os.path.join(HERE, "skeleton_knn_ref.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
