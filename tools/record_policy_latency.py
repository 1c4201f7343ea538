"""Record tests/golden/policy_latency.npz: the arrays tests/test_gpu_policy_latency.py
expects, from the library of the commit BEFORE a change to k_policy_act (never from the
build under test):

    git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
    BGX_LIB=../parent/mlp-ppo-2ply-p3_amd/bgx/libbgx.so python tools/record_policy_latency.py [OUT.npz]

BGX_LIB must be set: the in-tree library is the build under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mlp-ppo-2ply-p3_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    if not os.environ.get("BGX_LIB"):
        raise SystemExit("set BGX_LIB to the parent commit's libbgx.so")
    import test_gpu_policy_latency as T

    def golden(name):
        return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN_NPZ
    arrays = T.expected(golden)
    np.savez_compressed(out, **arrays)
    print(out, len(arrays), "arrays", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
