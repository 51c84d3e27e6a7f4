"""Writes tests/golden/textenc_{tiny,mid,full}.npz: the fixture ids of tests/textenc_restatement.py, the float64 restatement's
outputs on the seeded weights (which are regenerated from their seed and not stored: their checksum is), and e32 - the error of the
float32 torch.nn assembly on the CPU against those outputs, relative to max |output|, the unit of the GPU gate (4 * e32).

    python tools/capture_textenc_golden.py [tiny mid full]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import textenc_restatement as R  # noqa: E402


def main(names):
    for name in names or list(R.CONFIGS):
        c = R.case(name)
        out64 = R.forward(c["sd"], c["cfg"], c["ids"])
        e32 = R.float32_error(c["sd"], c["cfg"], c["ids"], out64)
        path = os.path.join(ROOT, "tests", "golden", f"textenc_{name}.npz")
        np.savez_compressed(path, ids=c["ids"], out64=out64, e32=np.float64(e32), weight_seed=np.int64(R.WEIGHT_SEED[name]),
                            state_checksum=np.array(R.state_checksum(c["sd"])))
        print(f"{name}: {path}: out {out64.shape}, max|out| = {np.abs(out64).max():.3f}, e32 = {e32:.3e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
