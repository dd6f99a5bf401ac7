#!/usr/bin/env python
"""Write tests/golden/xbd_split.json FROM scikit-learn (needs sklearn; no GPU): what the training scripts' line

    train_idxs0, val_idxs = train_test_split(np.arange(n), test_size=test_size, random_state=seed)

(xBD_code/train.py:409, train_unettransformer.py:508) returns, for tests/test_xbd_trainset_cpu.py to hold
datasets/xbd_pipeline.split_indices to without importing sklearn.  Per case of the grid NS x TEST_SIZES x SEEDS: the two index
lists in full for n <= FULL_UP_TO, otherwise their lengths and the SHA-256 of their little-endian int64 bytes (2799 is the
number of files of the xBD `train` folder, 9168 that of train + tier3).

    python tools/make_xbd_split_golden.py
"""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (2, 3, 4, 9, 10, 11, 19, 20, 21, 30, 31, 100, 2799, 9168)
TEST_SIZES = (0.1, 0.15)
SEEDS = (0, 10, 321)
FULL_UP_TO = 200


def digest(idxs):
    return hashlib.sha256(np.asarray(idxs).astype("<i8").tobytes()).hexdigest()


def main():
    import sklearn
    from sklearn.model_selection import train_test_split
    cases = []
    for n in NS:
        for test_size in TEST_SIZES:
            for seed in SEEDS:
                train, val = train_test_split(np.arange(n), test_size=test_size, random_state=seed)
                case = {"n": n, "test_size": test_size, "seed": seed, "n_train": len(train), "n_val": len(val)}
                if n <= FULL_UP_TO:
                    case.update(train=[int(i) for i in train], val=[int(i) for i in val])
                else:
                    case.update(train_sha256=digest(train), val_sha256=digest(val))
                cases.append(case)
    path = os.path.join(ROOT, "tests", "golden", "xbd_split.json")
    with open(path, "w") as f:
        json.dump({"sklearn": sklearn.__version__, "numpy": np.__version__, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
