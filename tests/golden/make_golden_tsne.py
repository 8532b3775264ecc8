"""Writes tests/golden/g_tsne.npz: what the reference's call,
sklearn.manifold.TSNE(n_components=2, learning_rate='auto', init='random', perplexity=p, random_state=s).fit_transform(x),
returns for the two end-to-end cases of tests/test_tsne_gpu.py, five seeds each, with the default (Barnes-Hut) method and with
method='exact'.  Run where sklearn is installed (python tests/golden/make_golden_tsne.py); the GPU tests import no sklearn.
Arrays only: <case>_default / <case>_exact [5, N, 2] f32, <case>_kl_default / <case>_kl_exact [5] f64 (sklearn's own
kl_divergence_), seeds [5], sklearn_version."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_ref as R  # noqa: E402

CASES = {"a": dict(N=300, D=40, K=6, perplexity=30.0, seed=0), "b": dict(N=257, D=40, K=5, perplexity=10.0, seed=1)}
SEEDS = (0, 1, 2, 3, 4)


def main():
    import sklearn
    from sklearn.manifold import TSNE
    out = {"seeds": np.asarray(SEEDS, np.int64), "sklearn_version": np.asarray(sklearn.__version__)}
    for name, c in CASES.items():
        x, _ = R.blobs(c["N"], c["D"], c["K"], c["seed"])
        for method, key in (("barnes_hut", "default"), ("exact", "exact")):
            ys, kls = [], []
            for s in SEEDS:
                t = TSNE(n_components=2, learning_rate='auto', init='random', perplexity=c["perplexity"], random_state=s, method=method)
                ys.append(t.fit_transform(x).astype(np.float32))
                kls.append(float(t.kl_divergence_))
                print(name, key, s, kls[-1], flush=True)
            out[f"{name}_{key}"] = np.stack(ys)
            out[f"{name}_kl_{key}"] = np.asarray(kls, np.float64)
    np.savez_compressed(os.path.join(HERE, "g_tsne.npz"), **out)


if __name__ == "__main__":
    main()
