"""The few-shot linear probe on the device: feature banks, shot selection, and the C search of the reference's linear_probe.py
over a batched logistic solver (csrc/logreg.hip) instead of 1 150 sklearn fits per dataset.

    features, labels = extract_features(model.point_encoder, loader)          # lp_feat_extractor.py:44-60
    save_features("train.npz", features, labels)                               # lp_feat_extractor.py:64-68 (same keys)
    result = linear_probe(load_features("train.npz"), load_features("test.npz"))
    python -m ppt_amd.probe --train train.npz --test test.npz [--num_run 10 --num_step 8 --out DIR]

What is promised and what is not: the selections are the reference's draws bit for bit, the search follows its rules
on the accuracies measured here, and every fit meets sklearn's stationarity criterion max |grad (F / n)| <= tol with the intercept
at its exact optimum for the returned W.  Where sklearn's answer is an artefact of where its optimiser stopped -- C >= 1e2 on
separable few-shot data, and C <= 1e-4, where the intercept decides and sklearn's is not converged -- the accuracies here differ
from the reference's.
"""
import argparse
import os

import numpy as np
import torch

from . import ops

SEARCH_LIST = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]          # linear_probe.py:52
VAL_SHOTS = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}                  # linear_probe.py:23


def extract_features(point_encoder, batches):
    """point_encoder(pc) over every batch (the short last one too), in eval mode under no_grad, as lp_feat_extractor.py:44-60.
    `batches`: any iterable of (pc, label, ...) -- a DataLoader, DevicePrefetcher, DeviceBatchLoader or a list.  The precision
    mode is the caller's; the training flag is restored.  -> (features [N, D] f32 on the device, labels [N] i64 on the device)"""
    was_training = point_encoder.training
    point_encoder.eval()
    feats, labels = [], []
    try:
        with torch.no_grad():
            for item in batches:
                pc, label = item[0], item[1]
                feature = point_encoder(pc.cuda(non_blocking=True))                  # lp_feat_extractor.py:54-55
                feats.append(feature.float())
                labels.append(torch.as_tensor(label).to(feature.device, torch.int64).reshape(-1))
    finally:
        point_encoder.train(was_training)
    if not feats:
        raise ValueError("extract_features: no batches")
    return torch.cat(feats).contiguous(), torch.cat(labels)


def save_features(path, features, labels):
    """the reference's bank file (lp_feat_extractor.py:64-68): keys feature_list, label_list; np.savez appends .npz"""
    np.savez(path, feature_list=torch.as_tensor(features).detach().cpu().numpy(), label_list=torch.as_tensor(labels).cpu().numpy())


def load_features(path):
    """-> (features f32 [N, D], labels i64 [N]) as numpy; accepts the float64 lists the reference writes"""
    with np.load(path) as f:
        return np.ascontiguousarray(f["feature_list"], dtype=np.float32), np.asarray(f["label_list"]).astype(np.int64)


def select_shots(train_labels, val_labels, num_shot, seed):
    """The reference's draws (linear_probe.py:28-46): np.random.seed(seed); for each label in np.unique order a choice without
    replacement among its rows, every train draw before any validation draw.  Host numpy -> (train_idx, val_idx) int64."""
    train_labels, val_labels = np.asarray(train_labels), np.asarray(val_labels)
    np.random.seed(seed)
    all_labels = np.unique(train_labels)
    train_idx, val_idx = [], []
    for label in all_labels:
        train_idx.extend(np.random.choice(np.where(train_labels == label)[0], size=num_shot, replace=False))
    for label in all_labels:
        val_idx.extend(np.random.choice(np.where(val_labels == label)[0], size=VAL_SHOTS[num_shot], replace=False))
    return np.array(train_idx, np.int64), np.array(val_idx, np.int64)


def _device_bank(bank):
    feat, labels = bank
    feat = torch.as_tensor(feat).to("cuda", torch.float32).contiguous()
    return feat, torch.as_tensor(labels).to("cuda", torch.int64).contiguous()


class DeviceFit:
    """The batched fit-and-score of the protocol: one solver launch and one prediction launch per call.

        fit(train_rows [R, n], val_rows [R, nv], Cs [R, G]) -> (val_acc [R, G], test_acc [R, G], coef)

    Run r's G fits use the rows train_rows[r] of the train bank; each is scored on the rows val_rows[r] of the test bank (the
    validation pool is the test bank, linear_probe.py:21) and on the whole test bank.  Accuracies are fractions, counted on the
    device and read with one transfer.  coef = dict(W [R, G, K, d], b [R, G, K], info [R, G, 8]) device tensors."""

    def __init__(self, train, test, tol=1e-4, max_iter=1000):
        self.train_feat, self.train_labels = _device_bank(train)
        self.test_feat, self.test_labels = _device_bank(test)
        classes = torch.unique(self.train_labels)
        self.K = int(classes.numel())
        if not torch.equal(classes, torch.arange(self.K, device=classes.device)):
            raise ValueError("linear probe: labels must be 0 .. K-1")              # (the reference's datasets number them so)
        self.tol, self.max_iter = tol, max_iter
        self.launches = []          # (fits, rows per fit, info records on the device) per call, for tools/linprobe_time.py
        self._ws = None

    def __call__(self, train_rows, val_rows, Cs):
        Cs = np.asarray(Cs, np.float64)
        R, G = Cs.shape
        dev = self.train_feat.device
        rows = torch.as_tensor(np.repeat(np.asarray(train_rows), G, axis=0).astype(np.int32), device=dev)          # [R G, n]
        d = self.train_feat.shape[1]
        need = ops.logreg_workspace_bytes(R * G, rows.shape[1], d, self.K)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        W, b, info = ops.logreg_fit(self.train_feat, self.train_labels, rows, Cs.reshape(-1), self.K, tol=self.tol,
                                    max_iter=self.max_iter, workspace=self._ws)
        self.launches.append((R * G, rows.shape[1], info))
        pred = ops.logreg_predict(self.test_feat, W, b)                                                           # [R G, Ntest]
        hit = (pred == self.test_labels[None, :]).view(R, G, -1)
        val = torch.as_tensor(np.asarray(val_rows), device=dev).long()                                            # [R, nv]
        val_acc = torch.gather(hit, 2, val[:, None, :].expand(R, G, -1)).double().mean(2)
        out = torch.stack([val_acc, hit.double().mean(2)]).cpu().numpy()                                          # the one transfer
        self.last_info = info.view(R, G, -1)
        return out[0], out[1], dict(W=W.view(R, G, self.K, d), b=b.view(R, G, self.K), info=self.last_info)


def linear_probe(train, test, shots=(1, 2, 4, 8, 16), num_run=10, num_step=8, tol=1e-4, max_iter=1000, fit=None,
                 out_dir=None, dataset="modelnet40", tag=None, keep_coef=False):
    """The protocol of linear_probe.py:23-117 on two feature banks (features [N, D], labels [N]; numpy or tensors).

    For each shot count all num_run seeds advance together: one launch fits the 7-point grid of every seed (7 num_run fits), the
    first maximal validation accuracy names c_peak (np.argmax, :63), the range starts at [c_peak / 10, 10 c_peak] (:65); each of
    the num_step steps fits both ends for every seed (2 num_run fits), keeps the right end only if it is strictly better (:79),
    scores the kept end on the whole test bank (:92-93) and halves the range in log10 towards it (:83-90).
    `fit`: the batched fit-and-score, see DeviceFit (default: DeviceFit(train, test, tol, max_iter)).
    -> dict(steps={shot: [per seed: [per step: (C, test accuracy in percent)]]}, summary={shot: (mean, population std) of the
    last step's accuracies}, selections={shot: [per seed: (train_idx, val_idx)]}, lines=(detail lines, summary lines)[, coef]).
    With out_dir the two text files of :97-120 are appended to, in the reference's formats."""
    train_labels = np.asarray(torch.as_tensor(train[1]).cpu())
    test_labels = np.asarray(torch.as_tensor(test[1]).cpu())
    if fit is None:
        fit = DeviceFit(train, test, tol, max_iter)
    tag = tag or {"modelnet40": "mn40", "scanobjectnn": "sonn"}.get(dataset, dataset)          # linear_probe.py:13
    result = dict(steps={}, summary={}, selections={}, val={}, coef={}, lines=([], []))
    for num_shot in shots:
        sel = [select_shots(train_labels, test_labels, num_shot, seed) for seed in range(1, num_run + 1)]      # seed = run id, :27
        train_rows, val_rows = np.stack([s[0] for s in sel]), np.stack([s[1] for s in sel])
        val_acc, _, _ = fit(train_rows, val_rows, np.tile(np.array(SEARCH_LIST), (num_run, 1)))
        peak = np.argmax(val_acc, axis=1)                                                                       # first maximum, :63
        c_left = np.array([1e-1 * SEARCH_LIST[p] for p in peak])                                                # :65
        c_right = np.array([1e1 * SEARCH_LIST[p] for p in peak])
        steps = [[] for _ in range(num_run)]
        coefs = [[] for _ in range(num_run)]
        details = [[] for _ in range(num_run)]          # written seed by seed, as the reference's loop order does
        vals = [dict(grid=val_acc[r].tolist(), steps=[]) for r in range(num_run)]
        for step in range(num_step):
            val_acc, test_acc, coef = fit(train_rows, val_rows, np.stack([c_left, c_right], 1))
            for r in range(num_run):
                right = bool(val_acc[r, 0] < val_acc[r, 1])                                                      # strict: a tie goes left, :79
                c_final = c_right[r] if right else c_left[r]
                log_l, log_r = np.log10(c_left[r]), np.log10(c_right[r])
                if right:                                                                                       # :83-84
                    log_l, log_r = 0.5 * (log_r + log_l), log_r
                else:                                                                                           # :89-90
                    log_l, log_r = log_l, 0.5 * (log_r + log_l)
                c_left[r], c_right[r] = np.power(10, log_l), np.power(10, log_r)                                # :102-103
                acc = 100 * float(test_acc[r, int(right)])                                                      # :93
                steps[r].append((float(c_final), acc))
                vals[r]["steps"].append((float(val_acc[r, 0]), float(val_acc[r, 1])))
                if keep_coef and coef is not None:
                    coefs[r].append((coef["W"][r, int(right)].cpu(), coef["b"][r, int(right)].cpu()))
                details[r].append("{}, seed {}, {} shot, weight {}, test_acc {:.2f}\n".format(dataset, r + 1, num_shot, c_final, acc))      # :97
        result["lines"][0].extend(line for per_seed in details for line in per_seed)
        last = np.array([s[-1][1] for s in steps]) if num_step else np.zeros(num_run)
        result["steps"][num_shot], result["selections"][num_shot], result["val"][num_shot] = steps, sel, vals
        if keep_coef:
            result["coef"][num_shot] = coefs
        result["summary"][num_shot] = (float(np.mean(last)), float(np.std(last)))                                # :114-115
        result["lines"][1].append("{}, {} Shot, Test acc stat: {:.2f} ({:.2f})\n".format(dataset, num_shot, *result["summary"][num_shot]))      # :116
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for name, lines in (("{}-run{}-step{}_details.txt".format(tag, num_run, num_step), result["lines"][0]),      # :98
                            ("{}-run{}-step{}.txt".format(tag, num_run, num_step), result["lines"][1])):               # :118
            with open(os.path.join(out_dir, name), "a+") as writer:
                writer.writelines(lines)
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description="few-shot linear probe on two feature banks (.npz: feature_list, label_list)")
    ap.add_argument("--train", required=True)
    ap.add_argument("--test", required=True)
    ap.add_argument("--num_run", type=int, default=10)
    ap.add_argument("--num_step", type=int, default=8)
    ap.add_argument("--dataset_name", default="modelnet40")
    ap.add_argument("--out", default=None, help="directory for the reference's two text files")
    a = ap.parse_args(argv)
    res = linear_probe(load_features(a.train), load_features(a.test), num_run=a.num_run, num_step=a.num_step,
                       out_dir=a.out, dataset=a.dataset_name)
    print("".join(res["lines"][1]), end="")
    return res


if __name__ == "__main__":
    main()
