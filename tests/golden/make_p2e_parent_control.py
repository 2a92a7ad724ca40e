#!/usr/bin/env python3
"""Recording of the categorical fused Plan2Explore update as it was BEFORE the continuous-latent route existed
(commit 864ae88, "Fused Plan2Explore update: member-batched ensemble kernels and replay"), for the control test
tests/test_gauss_p2e_gpu.py::test_categorical_update_is_unchanged.  Needs an MI355X and a checkout of that commit:

    git worktree add <dir> 864ae88 && (cd <dir> && python __graft_entry__.py)
    python <this file> <dir> <repository>/tests/golden/tiny_p2e_fused_parent.npz

It runs tests/test_p2e_fused_gpu.py's own `_update("tiny_p2e", fused=True, profile=True)` of that checkout twice, prints
ops.PROFILE's launch count (153 when recorded: PARENT_LAUNCHES in the test), checks that the two runs agree bit for bit,
and stores every parameter of the Plan2Explore module after the update (the world model's excluded).  Data only."""
import os
import sys

import numpy as np


def main():
    root, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    sys.path[:0] = [root, os.path.join(root, "dreamerv3-torch_amd")]
    import dv3hip
    from tests.test_p2e_fused_gpu import _update

    assert os.path.abspath(dv3hip.__file__).startswith(root), dv3hip.__file__
    runs = []
    for _ in range(2):
        run = _update("tiny_p2e", fused=True, profile=True)
        print("library launches:", sum(v["launches"] for v in run["launches"].values()))
        runs.append({k: v.cpu().numpy() for k, v in run["p2e"].state_dict().items()
                     if not k.startswith(("_behavior._world_model.", "actor."))})
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0]), "the update is not reproducible run to run"
    np.savez_compressed(out, **runs[0])
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
