"""The hallucination gate without a GPU: the threshold calibration's host part against sklearn and against a hand-worked
table, the constructor's and the C ABI's argument checks, the lazy export, and self-checks of the oracle
(tests/classifier_ref.py) that the GPU tests lean on."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi

import classifier_ref as cref

MRI = dict(data="mri", mean_flair=310.0, std_flair=420.0, mean_t1=505.0, std_t1=380.0)

# (scores, labels, threshold), worked by hand from the ROC points (fps, tps) per distinct score, descending:
TABLE = [
    # (0,1) (1,1) (1,2) (2,2): TPR - FPR = 0 | .5 0 .5 0 -> the first maximum, at score 0.8
    ([0.1, 0.4, 0.35, 0.8], [0, 0, 1, 1], 0.8),
    # (1,0) (1,1): TPR - FPR = 0 | -1 0 -> the leading (0, 0) point wins: +inf, nothing is ever accepted
    ([0.9, 0.1], [0, 1], float("inf")),
    # perfectly separable: (0,1) (0,2) (1,2) (2,2); the point at 0.7 lies on the line to (2,2) and is dropped; max at 0.8
    ([0.9, 0.8, 0.7, 0.6], [1, 1, 0, 0], 0.8),
    # ties, P = N = 5: (2,1) (2,3) (3,4) (4,5) (5,5) at scores 5 4 2 1 0.  (3,4) is collinear with its neighbours and
    # dropped.  TPR - FPR: 4 -> .6 - .4 = 0.19999999999999996, 2 -> .8 - .6 = 0.20000000000000007 (equal on paper), 1 ->
    # 1 - .8 = 0.19999999999999996: with the drop the first maximum is at 4, without it the answer would be 2
    ([2, 4, 5, 0, 1, 4, 1, 2, 5, 5], [1, 1, 0, 0, 1, 1, 0, 0, 1, 0], 4.0),
    # all scores equal: one point (2,2) -> 0 | 0: +inf
    ([3.0, 3.0, 3.0, 3.0], [0, 1, 0, 1], float("inf")),
]


def _youden():
    from localdiffusion_hallucination_amd.classifier import youden_threshold
    return youden_threshold


@pytest.mark.parametrize("scores,labels,want", TABLE)
def test_youden_threshold_hand_worked(scores, labels, want):
    got = _youden()(np.asarray(scores, dtype=np.float64), np.asarray(labels))
    assert got == want
    s32 = np.asarray(scores, dtype=np.float32).reshape(-1, 1)            # fp32 scores, [N, 1] as the reference stacks them
    assert _youden()(s32, np.asarray(labels).reshape(-1, 1)) == float(np.float32(want))


def test_youden_threshold_rejects_bad_input():
    y = _youden()
    for labels in ([0, 0, 0], [1, 1, 1]):
        with pytest.raises(ValueError, match="both"):
            y(np.array([0.1, 0.2, 0.3]), np.array(labels))
    with pytest.raises(ValueError):
        y(np.array([0.1, 0.2]), np.array([0, 1, 1]))
    with pytest.raises(ValueError):
        y(np.array([0.1, np.nan]), np.array([0, 1]))
    with pytest.raises(ValueError):
        y(np.array([0.1, 0.2]), np.array([1, 2]))


def test_youden_threshold_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    y = _youden()

    def sk(s, lab, **kw):
        fpr, tpr, thr = metrics.roc_curve(lab + 1, s, pos_label=2, **kw)
        return float(thr[np.argmax(tpr - fpr)])

    r = np.random.default_rng(20240)
    n_inf = n_tied = n_drop = 0
    for case in range(3000):
        n = int(r.integers(2, 40))
        lab = r.integers(0, 2, n)
        if lab.sum() in (0, n):
            lab[0], lab[1] = 0, 1
        if case % 3 == 0:
            s = r.integers(0, 6, n).astype(np.float32)                      # heavy ties
        elif case % 3 == 1:
            s = np.round(r.normal(lab * 0.7, 1.0), 1).astype(np.float32)    # some ties, classes partly separated
        else:
            s = r.normal(lab * 1.5, 1.0).astype(np.float32)                 # continuous
        want = sk(s, lab)
        assert y(s, lab) == want, (case, s.tolist(), lab.tolist())
        n_inf += want == np.inf
        n_tied += len(np.unique(s)) < n
        n_drop += want != sk(s, lab, drop_intermediate=False)
    print(f"youden_threshold == sklearn on 3000 cases: {n_tied} with ties, {n_inf} at +inf, {n_drop} where the collinear drop decides")
    assert n_inf > 0 and n_tied > 500                          # the hard cases did occur
    for s, lab, want in TABLE:                                 # and the hand-worked table is sklearn's answer too
        assert sk(np.asarray(s, dtype=np.float64), np.asarray(lab)) == want
    # cases where the collinear drop decides are rare among random ones (about 1 in 2000): three known ones
    for s, lab in (TABLE[3][:2], ([1, 3, 5, 3, 3, 0, 1, 2, 3, 2], [1, 1, 0, 1, 0, 0, 0, 1, 1, 0]),
                   ([5, 5, 3, 2, 5, 1, 1, 4, 3, 4], [1, 1, 1, 0, 1, 0, 0, 1, 0, 0])):
        s, lab = np.asarray(s, dtype=np.float32), np.asarray(lab)
        assert y(s, lab) == sk(s, lab) != sk(s, lab, drop_intermediate=False)


def test_lazy_export():
    assert "PatchCoreClassifier" in ldh.__all__
    from localdiffusion_hallucination_amd.classifier import PatchCoreClassifier
    assert ldh.PatchCoreClassifier is PatchCoreClassifier
    code = ("import sys, localdiffusion_hallucination_amd as m; "
            "bad = [k for k in sys.modules if k.startswith(m.__name__ + '.') and k.rsplit('.', 1)[1] in "
            "('classifier', 'patchcore', '_cabi', 'diffusion', 'unet')]; "
            "assert not bad, bad; assert m.PatchCoreClassifier.__name__ == 'PatchCoreClassifier'")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


def test_constructor_validation():
    pc84, pc224 = ldh.PatchCore((84, 84)).eval(), ldh.PatchCore((224, 224)).eval()
    K = ldh.PatchCoreClassifier
    with pytest.raises(ValueError, match="threshold"):
        K(dict(data="mnist"), 3, pc84)
    with pytest.raises(ValueError, match="input_size"):
        K(dict(data="mnist"), 3, pc224, threshold=1.0)
    with pytest.raises(ValueError, match="input_size"):
        K(dict(data="mvtec_pill"), "pill", pc84, threshold=1.0)
    with pytest.raises(ValueError, match="input_size"):
        K(dict(data="mnist"), 3, ldh.PatchCore((84, 96)).eval(), threshold=1.0)
    with pytest.raises(ValueError, match="std_t1"):
        K({k: v for k, v in MRI.items() if k != "std_t1"}, "t1", pc224, threshold=1.0)
    with pytest.raises(ValueError, match="mean_flair"):
        K(dict(data="mri"), "flair", pc224, threshold=1.0)
    for cfg, obj, pc in ((dict(data="mnist"), 3, pc84), (dict(data="mvtec_pill"), "pill", pc224), (MRI, "flair", pc224)):
        clf = K(cfg, obj, pc, threshold=float("inf"), return_map=False)
        assert clf.threshold == float("inf") and clf.patchcore is pc
        with pytest.raises(ValueError, match="predict"):
            clf(torch.zeros(2, 1, 32, 32))
        with pytest.raises(ValueError):
            clf.predict(torch.zeros(1, 2, 32, 32))
    mini = (0 - MRI["mean_flair"]) / MRI["std_flair"]
    assert K(MRI, "flair", pc224, threshold=0.0).affine == (mini, 420.0, 310.0, 4096.0)
    assert K(MRI, "anything else", pc224, threshold=0.0).affine == ((0 - 505.0) / 380.0, 380.0, 505.0, 4096.0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_gate_fails_loudly_without_gpu():
    clf = ldh.PatchCoreClassifier(dict(data="mnist"), 3, ldh.PatchCore((84, 84)).eval(), threshold=1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        clf(torch.zeros(1, 1, 28, 28))


def test_loader_builds_the_mode_size(tmp_path):
    from localdiffusion_hallucination_amd import checkpoint, weights
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    bank = np.arange(4 * 1536, dtype=np.float32).reshape(4, 1536)
    clf = checkpoint.load_patchcore_classifier(sd, bank, dict(data="mvtec_all"), "tile", threshold=40.0, device="cpu")
    assert clf.patchcore.input_size == (224, 224) and clf.patchcore.num_neighbors == 9 and not clf.patchcore.training
    assert torch.equal(clf.patchcore.memory_bank, torch.from_numpy(bank))
    # the reference's mnist checkpoint: one state_dict of the whole module, the bank inside
    whole = {"feature_extractor." + k: v for k, v in sd.items()}
    whole["memory_bank"] = torch.from_numpy(bank[:3])
    clf = checkpoint.load_patchcore_classifier(whole, None, dict(data="mnist"), 3, threshold=40.0, device="cpu")
    assert clf.patchcore.input_size == (84, 84) and clf.patchcore.memory_bank.shape == (3, 1536)
    with pytest.raises(RuntimeError, match="memory bank"):
        checkpoint.load_patchcore_classifier(sd, None, dict(data="mnist"), 3, threshold=40.0, device="cpu")
    with pytest.raises(ValueError, match="threshold"):
        checkpoint.load_patchcore_classifier(sd, bank, dict(data="mnist"), 3, device="cpu")


def test_cabi_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    assert lib.ld_clf_max(None, 1, 16, None, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_clf_max(1, 0, 16, 1, None) == -1
    assert lib.ld_clf_max(1, 1, 0, 1, None) == -1
    assert lib.ld_clf_decide(None, 1.0, None, 1, None) == -1
    assert lib.ld_clf_decide(1, 1.0, 1, 0, None) == -1
    assert lib.ld_clf_resize(None, None) == -1

    def args(**kw):
        a = cabi.ClfResizeArgs()
        a.x = a.out = 1
        a.B, a.Cin, a.Cout, a.Hi, a.Wi, a.Ho, a.Wo = 1, 1, 3, 28, 28, 84, 84
        a.mode, a.normalize = cabi.CLF_PLAIN, 1
        for c in range(3):
            a.mean[c], a.std[c] = 0.5, 0.25
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad, word in ((dict(x=None), b"null"), (dict(out=None), b"null"), (dict(Cin=2), b"channels"),
                      (dict(Cin=4, Cout=4), b"Normalize"), (dict(B=0), b"sizes"), (dict(Hi=0), b"sizes"),
                      (dict(Wo=0), b"sizes"), (dict(mode=3), b"mode"), (dict(mode=cabi.CLF_HALVE), b"max words"),
                      (dict(mode=cabi.CLF_AFFINE), b"divisor"), (dict(n_zero=2), b"n_zero"), (dict(pred=1), b"decision")):
        assert lib.ld_clf_resize(C.byref(args(**bad)), None) == -1, bad
        assert word in lib.ld_last_error(), (bad, lib.ld_last_error())
    a = args()
    a.std[1] = 0.0
    assert lib.ld_clf_resize(C.byref(a), None) == -1 and b"std" in lib.ld_last_error()


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_ref_mri_affine():
    x = torch.tensor([[[[0.0, 1.0], [2.5, -0.5]]]])
    for obj, key in (("flair", "flair"), ("t1", "t1"), ("pill", "t1")):
        mean, std = MRI["mean_" + key], MRI["std_" + key]
        got = cref.mri_affine(x.double(), MRI, obj)
        want = ((x.double() + mean / std) * std + mean) / 4096.0        # x - mini = x + mean / std: NOT x - |mini|
        assert torch.allclose(got, want, rtol=1e-14, atol=0)
        assert float(got[0, 0, 0, 0]) == pytest.approx(2 * mean / 4096.0, rel=1e-14)
    y = cref.preprocess(x, MRI, "flair", size=4)
    assert y.shape == (1, 3, 4, 4) and y.dtype == torch.float32
    back = y * torch.tensor(cref.IMAGENET_STD).view(1, 3, 1, 1) + torch.tensor(cref.IMAGENET_MEAN).view(1, 3, 1, 1)
    assert torch.allclose(back[:, 0], back[:, 2], atol=1e-6)              # one channel, three times


def test_ref_halving_is_decided_on_the_whole_tensor():
    cfg = dict(data="mnist")
    x = torch.full((2, 1, 28, 28), 0.5)
    x[1, 0, 27, 27] = 1.5                                                 # only the last value of the last sample
    whole = cref.preprocess(x, cfg, 3)
    per = cref.preprocess(x, cfg, 3, per_sample_max=True)
    alone = cref.preprocess(x[:1], cfg, 3)
    assert whole.shape == (2, 3, 84, 84)
    assert torch.equal(per[:1], alone) and not torch.equal(whole[:1], alone)
    assert torch.equal(whole[1:], per[1:])
    std, mean = torch.tensor(cref.IMAGENET_STD).view(1, 3, 1, 1), torch.tensor(cref.IMAGENET_MEAN).view(1, 3, 1, 1)
    assert torch.allclose(whole[:1] * std + mean, torch.full((1, 3, 84, 84), 0.25), atol=1e-6)
    assert torch.allclose(alone * std + mean, torch.full((1, 3, 84, 84), 0.5), atol=1e-6)
    x[1, 0, 27, 27] = 1.0                                                 # max == 1.0 is not above 1.0
    assert torch.equal(cref.preprocess(x, cfg, 3)[:1], alone)
