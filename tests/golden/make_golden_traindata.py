#!/usr/bin/env python3
"""Golden vectors for the query sampler of the training-data generator (posendf_amd.traindata.sample_queries), produced by the
REFERENCE itself: data/create_data.py PoseData.__getitem__ in mode 'query' under np.random.seed(s), on a seeded synthetic
`pose_body` file (tests/knn_oracle.make_pose_body).  The module imports faiss, smplx, pytorch3d and ipdb at the top: they are
stubbed, and pytorch3d's axis_angle_to_quaternion is the engine's restatement (posendf_amd.motion_denoise), so both sides start
from the same quaternions.  Only the outputs are stored.   usage: python tests/golden/make_golden_traindata.py"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from knn_oracle import make_pose_body  # noqa: E402
from posendf_amd.motion_denoise import axis_angle_to_quaternion  # noqa: E402

for name in ("faiss", "ipdb", "pytorch3d", "smplx"):
    sys.modules[name] = types.ModuleType(name)
for cls in ("SMPL", "SMPLH", "SMPLX"):
    setattr(sys.modules["smplx"], cls, None)
tr = types.ModuleType("pytorch3d.transforms")
tr.axis_angle_to_quaternion = axis_angle_to_quaternion
sys.modules["pytorch3d.transforms"] = tr
sys.path.insert(0, "/root/reference/data")
import create_data  # noqa: E402

SEQ = dict(n=300, seed=3, width=69)          # the synthetic sequence file
SEEDS = (0, 1, 2)
NUM_SAMPLES = (100, 45)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "seq.npz")
        np.savez(path, pose_body=make_pose_body(**SEQ))
        for n in NUM_SAMPLES:
            data = create_data.PoseData(path, mode="query", num_samples=n)
            for s in SEEDS:
                np.random.seed(s)
                items = [data[i]["pose"] for i in range(2)]        # two items from one stream
                out[f"pose_n{n}_s{s}"] = np.stack(items)
    np.savez_compressed(os.path.join(HERE, "traindata_sampler.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
