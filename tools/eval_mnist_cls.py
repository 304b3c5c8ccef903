#!/usr/bin/env python3
"""The hallucination read-out of the MNIST experiment: which digit does the classifier see in the super-resolved images,
and which in the HR images they should equal?  An "8" restored by a model trained on "3"s that reads as a 3 is a
hallucination the MSE does not show.

Reads a ``pred_all.npy`` / ``hr_all.npy`` pair as tools/run_eval.py writes them ([N, 1, 28, 28] in [0, 2]) and the true
labels ([N], a .npy file, an idx(.gz) file, or one digit for all images), and a classifier checkpoint
(tools/train_mnist_cls.py, or the reference's train_mnist_cls.py:116).

  python tools/eval_mnist_cls.py --dir results/cfg1 --labels 8 --model results/mnist_cls/mnist_cls_best_model.pth
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                                   # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, evalio                 # noqa: E402


def read_labels(spec, n):
    if spec.isdigit():
        return np.full(n, int(spec), np.int64)
    y = np.load(spec) if spec.endswith(".npy") else evalio.read_idx(spec)
    y = np.asarray(y).astype(np.int64).reshape(-1)
    if y.shape[0] < n:
        raise SystemExit(f"--labels: {y.shape[0]} labels for {n} images")
    return y[:n]


def show(name, rep):
    print(f"{name}: accuracy {100 * rep['accuracy']:.2f} % of {int(rep['confusion'].sum())}")
    print("  rows = true digit, columns = predicted")
    for d, row in enumerate(rep["confusion"]):
        if row.sum():
            print(f"  {d}: " + " ".join(f"{v:5d}" for v in row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="directory holding pred_all.npy and hr_all.npy")
    ap.add_argument("--labels", required=True)
    ap.add_argument("--model", required=True)
    ap.add_argument("--trust-pickle", action="store_true")
    a = ap.parse_args()
    pred, hr = np.load(os.path.join(a.dir, "pred_all.npy")), np.load(os.path.join(a.dir, "hr_all.npy"))
    pred = pred.reshape(-1, 1, pred.shape[-2], pred.shape[-1])[:, -1:]
    hr = hr.reshape(-1, 1, hr.shape[-2], hr.shape[-1])
    if pred.shape != hr.shape or tuple(hr.shape[1:]) != (1, 28, 28):
        raise SystemExit(f"pred_all {pred.shape} / hr_all {hr.shape}: expected matching [N, 1, 28, 28]")
    y = read_labels(a.labels, hr.shape[0])
    net = ldh.MnistClassifier()
    print("model:", checkpoint.load_mnist_classifier(a.model, net, trust_pickle=a.trust_pickle))
    net = net.to("cuda")
    rep_pred, rep_hr = evalio.digit_report(net, pred, y), evalio.digit_report(net, hr, y)
    show("prediction", rep_pred)
    show("HR", rep_hr)
    changed = int((rep_pred["pred"] != rep_hr["pred"]).sum())
    print(f"images whose predicted digit differs between the prediction and HR: {changed} of {hr.shape[0]}")


if __name__ == "__main__":
    main()
