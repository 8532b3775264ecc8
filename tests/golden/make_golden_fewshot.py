#!/usr/bin/env python3
"""Generate tests/golden/g_fewshot.npz: what the UPSTREAM REFERENCE's generate_fewshot_dataset (data/dataset_3d.py:210-254,
imported through tests/golden/ref_import.py) selects from a small label vector, for ppt_amd/data/fewshot.py.  Build container
only; only arrays are stored.

    python tests/golden/make_golden_fewshot.py

50 labels over 7 classes with unequal counts (two classes hold fewer than 9 items, one fewer than 4), in an order in which the
classes do not first appear sorted.  Per (seed, shots) in {0, 3} x {1, 4, 9} the reference runs after random.seed(seed), as it
does after set_random_seed; with 9 shots the short classes take its random.choices branch.  Also stored: repeat=False at 9
shots, num_shots=-1, and the selection drawn from the GLOBAL stream (the seed=None path).
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_import as R                     # noqa: E402

COUNTS = {4: 12, 1: 3, 6: 10, 0: 7, 3: 9, 5: 1, 2: 8}          # class -> items (50 in all)
SEEDS, SHOTS = (0, 3), (1, 4, 9)


def labels():
    lab = np.concatenate([np.full(n, c, np.int64) for c, n in COUNTS.items()])
    return lab[np.random.RandomState(7).permutation(lab.shape[0])]


def main():
    lab = labels()
    assert lab.shape[0] == 50 and len(set(lab.tolist())) == 7
    with R.reference_context():
        import data.dataset_3d as D
    source = [{"pc": None, "label": int(c), "classname": str(c), "index": i} for i, c in enumerate(lab)]
    out = {"labels": lab}

    def picked(**kw):
        return np.asarray([item["index"] for item in D.generate_fewshot_dataset(source, **kw)], dtype=np.int64)

    for seed in SEEDS:
        for shots in SHOTS:
            random.seed(seed)
            out[f"seed{seed}_shots{shots}"] = picked(num_shots=shots)
        random.seed(seed)
        out[f"seed{seed}_shots9_norepeat"] = picked(num_shots=9, repeat=False)
    out["all"] = picked(num_shots=-1)
    random.seed(11)                                     # two selections in a row from the global stream
    out["global_seed11_shots4_then_2"] = np.concatenate([picked(num_shots=4), picked(num_shots=2)])
    path = os.path.join(HERE, "g_fewshot.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
