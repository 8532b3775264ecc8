"""The K-shot training sets of the `*_fs` datasets (data/dataset_3d.py:210-254: generate_fewshot_dataset over
split_dataset_by_label), as dataset INDICES: the selection needs the labels alone, the clouds stay where they are
(DeviceCloudSet.subset).

    idx = fewshot_indices(train_labels, num_shots=16, seed=args.seed)
    train_set = DeviceCloudSet(points, labels).subset(idx)
"""
import random

import numpy as np


def fewshot_indices(labels, num_shots, seed=None, repeat=True):
    """The items generate_fewshot_dataset(data_source, num_shots, repeat) keeps, as int64 indices into `labels`, bit for bit:
    classes in order of first appearance (the defaultdict of split_dataset_by_label), per class random.sample(items, num_shots),
    or -- a class with fewer items -- random.choices(items, k=num_shots) with `repeat` and all its items without.
    seed: the draws come from the stream random.seed(seed) starts (a private random.Random(seed): the same stream); None draws
    from the global `random` state, as the reference does after set_random_seed.  num_shots < 1: every index, in order."""
    labels = np.asarray(labels).reshape(-1)
    if num_shots < 1:
        return np.arange(labels.shape[0], dtype=np.int64)
    rng = random if seed is None else random.Random(seed)
    tracker = {}
    for i, label in enumerate(labels.tolist()):
        tracker.setdefault(int(label), []).append(i)
    picked = []
    for items in tracker.values():
        if len(items) >= num_shots:
            picked.extend(rng.sample(items, num_shots))
        elif repeat:
            picked.extend(rng.choices(items, k=num_shots))
        else:
            picked.extend(items)
    return np.asarray(picked, dtype=np.int64)
