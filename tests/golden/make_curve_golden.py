"""Writes tests/golden/curve_metrics_ped2.npz: scikit-learn's own values of the reference's `compute_eer` and
`precision_recall_auc` (main/eval_metric.py:315-379) at every 10th point of the ped2 fixture's 100 x 20 grid, at ped2's
published pair (test_helper.py:565-569) and at five synthetic cases with ties, so that the tests need no scikit-learn.
The normal class is the positive one (pos_label = 0).

    python tests/golden/make_curve_golden.py          (needs scikit-learn; written with 1.7.2)
"""
import os
import sys

import numpy as np
from sklearn import metrics

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fusion_cases as FC  # noqa: E402

# (n, k, decimals, seed, weight vector, smoothing pair) of FC.synthetic(n, k, seed=seed, decimals=decimals)
SYNTHETIC = [(65, 2, 1, 3, 0, 1), (65, 2, 1, 3, 1, 2), (300, 1, 1, 4, 0, 1), (1025, 4, 2, 5, 2, 0), (5000, 2, 2, 6, 3, 2)]


def cal_eer(fpr, tpr):
    return fpr[np.nanargmin(np.absolute(fpr + tpr - 1))]


def point(key, labels):
    """(eer on the full curve, eer with sklearn's default vertex dropping, average precision, auc(recall, precision))"""
    full = metrics.roc_curve(labels, key, pos_label=0, drop_intermediate=False)
    kept = metrics.roc_curve(labels, key, pos_label=0)
    precision, recall, _ = metrics.precision_recall_curve(labels, key, pos_label=0)
    return (cal_eer(full[0], full[1]), cal_eer(kept[0], kept[1]), metrics.average_precision_score(labels, key, pos_label=0),
            metrics.auc(recall, precision))


def main():
    fx = FC.fixture()
    S = len(fx["smooth"])
    index = np.arange(0, len(fx["weights"]) * S, 10)
    grid = np.array([point(FC.scores(fx["chan"], fx["weights"][i // S], *fx["smooth"][i % S]), fx["labels"]) for i in index])
    l1, l2 = fx["golden"]["ped2"][0]
    lam = np.array(point(FC.scores(fx["chan"], np.array([1 - l1, l1], dtype=np.float32), *FC.pairs([l2])[0]), fx["labels"]))
    syn = []
    for n, k, decimals, seed, g, s in SYNTHETIC:
        c = FC.synthetic(n, k, seed=seed, decimals=decimals)
        labels = np.ones(n, dtype=np.int64)
        labels[c["pos"]] = 0
        syn.append(point(FC.scores(c["chan"], c["weights"][g], *c["smooth"][s]), labels))
    syn = np.array(syn)
    names = ("eer_full", "eer_drop", "ap", "pr_auc")
    out = {"grid_index": index.astype(np.int32), "syn_case": np.array(SYNTHETIC, dtype=np.int32), "lam_map": np.array([l1, l2])}
    out.update({f"lam_{nm}": np.float64(lam[i]) for i, nm in enumerate(names)})
    out.update({f"grid_{nm}": grid[:, i].astype(np.float64) for i, nm in enumerate(names)})
    out.update({f"syn_{nm}": syn[:, i].astype(np.float64) for i, nm in enumerate(names)})
    path = os.path.join(HERE, "curve_metrics_ped2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
