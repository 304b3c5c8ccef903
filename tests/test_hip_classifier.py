"""The hallucination gate on the GPU (classifier.py over csrc/classifier.hip and PatchCore) against the plain-torch
restatement of the reference's Classifier_PatchCore (tests/classifier_ref.py): the preprocessing and resize kernels with
the fp64 evaluation of the oracle as the yardstick, the whole classifier in its three modes, the calibration, and the
gate driving GaussianDiffusion's classifier-gated re-branching."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                              # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi                  # noqa: E402
from localdiffusion_hallucination_amd import rng, weights                   # noqa: E402
from localdiffusion_hallucination_amd.classifier import youden_threshold    # noqa: E402
from oracle import diffusion_ref                                            # noqa: E402

import classifier_ref as cref                                               # noqa: E402
import patchcore_ref as ref                                                 # noqa: E402
from hip_helpers import DEV, st                                             # noqa: E402

REL = 1e-3            # whole-model bound of tests/test_hip_patchcore.py (derivation there); the gate adds the preprocessing
TOL = 1e-3            # sampler parity bound of tests/test_hip_sampler.py
FLOOR = 1e-6          # test_embed's bound on the existing bilinear kernel: the floor where the reference's own error is tiny
MNIST = dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
MRI_CFG = dict(data="mri", mean_flair=200.0, std_flair=700.0, mean_t1=350.0, std_t1=650.0)
_SD = {}


def rnd(shape, key, lo=0.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, 4646, key, lo, hi))


def dist64(a, want64):
    """max |a - want64| / max |want64|, in fp64."""
    return float((a.detach().cpu().double() - want64).abs().max() / want64.abs().max())


def rel_err(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max() / b.double().abs().max())


def state_dict():
    if "sd" not in _SD:
        _SD["sd"] = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    return _SD["sd"]


def planted_bank(emb, B, seed=0):
    """As in tests/test_hip_patchcore.py: a bank with a clear nearest row for every embedding row (e_i + noise of norm
    2.0 .. 2.9, the image's patch p* at 3.0), a cluster of 8 rows around p*'s row (the support set, at 1.6 .. 2.65 from
    it) and 997 far rows, shuffled.  Returns (bank, p* per image)."""
    N, D = emb.shape
    P = N // B
    g = torch.Generator().manual_seed(seed)
    dist = 2.0 + 0.9 * torch.rand(N, generator=g)
    pstar = torch.randint(0, P, (B,), generator=g)
    dist[torch.arange(B) * P + pstar] = 3.0
    n = torch.randn(N, D, generator=g)
    rows = [emb + n / n.norm(dim=1, keepdim=True) * dist[:, None]]
    for b in range(B):
        c = torch.randn(8, D, generator=g)
        r = 1.5 + 0.15 * torch.arange(1, 9, dtype=torch.float32)
        rows.append(rows[0][b * P + pstar[b]] + c / c.norm(dim=1, keepdim=True) * r[:, None])
    rows.append(emb.mean(0) + 3.0 * torch.randn(997, D, generator=g))
    bank = torch.cat(rows)
    return bank[torch.randperm(bank.shape[0], generator=g)].contiguous(), pstar


def assert_determinate(emb, bank, want, pstar):
    """The set-up's margins, as test_patchcore_whole_model asserts them: every argmin and the argmax are determinate;
    and the embedding norms are in the regime REL was derived for (there 16-52 against planted distances of 2-3: the
    cancellation in |x|^2 - 2 x.y + |y|^2 is eps |x|^2 / d^2, in the fp32 reference as much as in the kernel; at |x| = 152
    the CPU reference is 2.6e-3 from the exact distances, and that goes with |x|^2: under REL / 2 below 152 sqrt(REL / 2 / 2.6e-3) = 66)."""
    assert float(emb.norm(dim=1).max()) < 152.0 * (0.5 * REL / 2.6e-3) ** 0.5
    top2 = torch.cdist(emb.double(), bank.double()).topk(2, largest=False).values
    assert (top2[:, 1] - top2[:, 0] > 0.2).all()
    assert torch.equal(want.argmax(1), pstar)


def patchcore(size, bank=None, num_neighbors=9):
    m = ldh.PatchCore((size, size), num_neighbors=num_neighbors)
    m.feature_extractor.load_state_dict(state_dict())
    if bank is not None:
        m.set_memory_bank(bank)
    return m.to(DEV).eval()


def gate_input(config, obj, C, H, B, kind, key):
    """x0 of the named kind: 'below' (max < 1), 'above' (values up to 2), 'last' (only the very last value above 1),
    'mri' (normalised intensities that de-normalise to the 12-bit range: mean .. 4096, so that PatchCore's input fills
    [mean / 4096, 1] as the other modes' fills [0, 1] -- a low-contrast input puts the embedding norms at 150 and the
    planted bank's distances of 2-3 out of the regime REL was derived for, |x| 16-52: there the fp32 reference itself is
    2.6e-3 from the exact distances)."""
    if kind == "mri":
        key_ = "flair" if obj == "flair" else "t1"
        mean, std = config["mean_" + key_], config["std_" + key_]
        return (0 - mean) / std + rnd((B, C, H, H), key, 0.0, 1.0) * ((4096.0 - mean) / std)
    x = rnd((B, C, H, H), key, 0.0, 2.0 if kind == "above" else 0.9)
    if kind == "last":
        x[-1, -1, -1, -1] = 1.5
    assert abs(float(x.max()) - 1.0) > 1e-6                    # the halving decision itself is exact: no input at the edge
    return x


# ------------------------------------------------------------------------------------------------ single kernels
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("config,obj,H", [(dict(data="mnist"), 3, 28), (dict(data="mnist"), 3, 40),
                                          (dict(data="mvtec_pill"), "pill", 256), (MRI_CFG, "flair", 256),
                                          (MRI_CFG, "t1", 256)])
def test_preprocess_kernel(config, obj, H, C):
    """x0 -> PatchCore's input against classifier_ref.  PyTorch computes the source coordinate in fp32; at coordinates up
    to 255 that rounding times the pixel difference dominates, and a kernel that orders the arithmetic differently is as
    far from the exact result as the reference is.  Yardstick: the fp64 evaluation of classifier_ref; the kernel may be
    at most 2 x the fp32 reference's own distance from it, + 1e-6 (two independent roundings of the same size)."""
    S = cref.input_size(config["data"])
    clf = ldh.PatchCoreClassifier(config, obj, patchcore(S), threshold=0.0)
    mri = config["data"] == "mri"
    for B in (1, 2):
        for kind in (("mri",) if mri else ("below", "above", "last")):
            for per in ((False,) if mri else (False, True)):
                x0 = gate_input(config, obj, C, H, B, kind, 10 * B + C)
                want32 = cref.preprocess(x0, config, obj, per_sample_max=per)
                want64 = cref.preprocess(x0.double(), config, obj, per_sample_max=per)
                got = clf.preprocess(x0.to(DEV), per_sample_max=per)
                assert got.shape == (B, 3, S, S) and got.dtype == torch.float32
                e_ref, e = dist64(want32, want64), dist64(got, want64)
                print(f"preprocess {config['data']} obj={obj} C={C} {H}->{S} B={B} {kind} per_sample={per}: reference fp32 "
                      f"vs fp64 {e_ref:.2e}, kernel vs fp64 {e:.2e} (bound {2 * e_ref + FLOOR:.2e}), kernel vs fp32 "
                      f"reference {rel_err(got, want32):.2e}")
                assert e <= 2 * e_ref + FLOOR
                if kind == "last" and B == 2:                    # the rule is global: sample 0 is halved by sample 1's max
                    alone = cref.preprocess(x0[:1], config, obj)
                    assert (rel_err(got[:1], alone) > 0.1) == (not per)


def test_preprocess_repeated_calls_and_odd_sizes():
    """The two sets of max words alternate and are cleared by the launch that does not read them: a below / above /
    below sequence through ONE plan decides each call on its own.  An output width that is no multiple of 4 takes the
    element-wise stores."""
    config = dict(data="mnist")
    clf = ldh.PatchCoreClassifier(config, 3, patchcore(84), threshold=0.0)
    xs = [gate_input(config, 3, 1, 28, 2, kind, 77 + i) for i, kind in enumerate(("below", "above", "below", "last", "below",
                                                                                "below", "above", "above"))]
    for i, x0 in enumerate(xs):
        for per in (False, True) if i % 2 else (True, False):
            got = clf.preprocess(x0.to(DEV), per_sample_max=per)
            want64 = cref.preprocess(x0.double(), config, 3, per_sample_max=per)
            assert dist64(got, want64) <= 2 * dist64(cref.preprocess(x0, config, 3, per_sample_max=per), want64) + FLOOR, (i, per)
    x = rnd((2, 1, 30, 23), 5, 10.0, 60.0)
    for Ho, Wo in ((17, 31), (45, 22), (30, 23)):
        want64 = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=False)
        want32 = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False)
        got = resize_plain(x, Ho, Wo)
        assert dist64(got, want64) <= 2 * dist64(want32, want64) + FLOOR


def resize_plain(x, Ho, Wo, pred=None, threshold=0.0):
    B, Cc, H, W = x.shape
    xd = x.to(DEV).contiguous()
    out = torch.full((B, Cc, Ho, Wo), float("nan"), device=DEV)
    a = cabi.ClfResizeArgs()
    a.x, a.out = xd.data_ptr(), out.data_ptr()
    a.B, a.Cin, a.Cout, a.Hi, a.Wi, a.Ho, a.Wo, a.mode = B, Cc, Cc, H, W, Ho, Wo, cabi.CLF_PLAIN
    dec = None
    if pred is not None:
        dec = torch.full((pred.numel(),), -7, dtype=torch.int32, device=DEV)
        a.pred, a.threshold, a.decision, a.n_decision = pred.data_ptr(), threshold, dec.data_ptr(), pred.numel()
    cabi.check(cabi.lib().ld_clf_resize(C.byref(a), st()), "clf_resize")
    return out if pred is None else (out, dec)


@pytest.mark.parametrize("S,H,B", [(84, 28, 1), (84, 28, 2), (224, 256, 1), (224, 256, 2)])
def test_resize_back_kernel(S, H, B):
    """The anomaly map back to the image size (models.py:427) vs F.interpolate, same yardstick as the preprocessing."""
    m = rnd((B, 1, S, S), 130 + B, 10.0, 60.0)
    want32 = cref.resize_back(m, H, H)
    want64 = cref.resize_back(m.double(), H, H)
    got = resize_plain(m, H, H)
    e_ref, e = dist64(want32, want64), dist64(got, want64)
    print(f"resize back {S}->{H} B={B}: reference fp32 vs fp64 {e_ref:.2e}, kernel vs fp64 {e:.2e} (bound {2 * e_ref + FLOOR:.2e})")
    assert e <= 2 * e_ref + FLOOR


def test_decision_kernels():
    """pred_score > threshold as int32, alone and inside the resize launch: strict comparison, +-inf thresholds."""
    pred = torch.tensor([1.0, 2.0, 2.0000002, 3.0, -1.0, 59.96], device=DEV)
    lib = cabi.lib()
    for thr in (2.0, float("inf"), float("-inf"), 59.96, -1.5):
        want = (pred > thr).to(torch.int32)
        dec = torch.full((pred.numel(),), -7, dtype=torch.int32, device=DEV)
        cabi.check(lib.ld_clf_decide(pred.data_ptr(), thr, dec.data_ptr(), pred.numel(), st()), "clf_decide")
        assert torch.equal(dec, want), thr
        _, dec2 = resize_plain(rnd((1, 1, 8, 8), 3), 4, 4, pred=pred, threshold=thr)
        assert torch.equal(dec2, want), thr


# ------------------------------------------------------------------------------------------------ the whole classifier
@pytest.mark.parametrize("config,obj,C,H,kind", [(dict(data="mnist"), 3, 1, 28, "above"),
                                                 (dict(data="mvtec_pill"), "pill", 3, 256, "above"),
                                                 (MRI_CFG, "flair", 1, 256, "mri")])
def test_whole_classifier(config, obj, C, H, kind):
    """(decision, anomaly_map, pred_score) at B = 1 with the reference's num_neighbors = 9 on a planted bank whose argmin
    and argmax margins are asserted: score and map within REL of classifier_ref, the decision equal on both sides of the
    reference score, and return_map=False the same decision and score bit for bit without the map."""
    sd = state_dict()
    S = cref.input_size(config["data"])
    x0 = gate_input(config, obj, C, H, 1, kind, 500 + H)
    with torch.no_grad():
        emb, _ = ref.embedding(ref.features(sd, cref.preprocess(x0, config, obj)))
    bank, pstar = planted_bank(emb, 1)
    _, want_map, want_score, _ = cref.classifier_forward(sd, bank, x0, config, obj, 0.0)
    want = ref.patchcore_forward(sd, bank, cref.preprocess(x0, config, obj), (S, S))
    assert_determinate(emb, bank, want["patch_scores"], pstar)
    clf = ldh.PatchCoreClassifier(config, obj, patchcore(S, bank), threshold=0.0)
    s_ref = float(want_score[0])
    for factor, want_dec in ((0.9, 1), (1.1, 0)):
        clf.threshold = factor * s_ref
        dec, amap, score = clf(x0.to(DEV))
        assert cref.classifier_forward(sd, bank, x0, config, obj, factor * s_ref)[0].tolist() == [want_dec]
        assert isinstance(dec, int) and dec == want_dec
        assert amap.shape == (1, 1, H, H) and score.shape == (1,) and amap.is_cuda and score.is_cuda
        e_map, e_score = rel_err(amap, want_map), rel_err(score, want_score)
        print(f"classifier {config['data']} {H}->{S}: anomaly_map rel err {e_map:.2e}, pred_score rel err {e_score:.2e} (bound {REL:.0e})")
        assert e_map < REL and e_score < REL
    nomap = ldh.PatchCoreClassifier(config, obj, clf.patchcore, threshold=clf.threshold, return_map=False)
    dec2, none, score2 = nomap(x0.to(DEV))
    assert none is None and dec2 == dec and torch.equal(score2, score)
    d3, m3, s3 = clf.predict(x0.to(DEV), return_map=False)
    assert m3 is None and d3.dtype == torch.int32 and d3.tolist() == [dec] and torch.equal(s3, score)


def batch_setup(per):
    """(x0 [3, 1, 28, 28] with only sample 1 above 1.0, bank, reference outputs, threshold) for per_sample_max = per.
    num_neighbors = 1 on a bank of clean images' rows (distances of tens against norms of the same order): score and map
    are continuous in the input, whatever the contrast of the halved samples, and the three scores are far apart."""
    sd, config = state_dict(), dict(data="mnist")
    x0 = gate_input(config, 3, 1, 28, 3, "below", 900)
    x0[1] = rnd((1, 28, 28), 333, 0.0, 2.0)
    x0[2] *= 0.7                                                     # (apart from sample 0 in either mode)
    bank = gate_bank(sd, [clean_image(j) for j in range(4)])
    _, m_ref, s_ref, x_ref = cref.classifier_forward(sd, bank, x0, config, 3, 0.0, num_neighbors=1, per_sample_max=per)
    order = s_ref.sort().values
    gaps = (order[1:] - order[:-1]) / order[1:]
    assert float(gaps.min()) > 10 * REL                              # rounding cannot reorder the scores
    i = int(gaps.argmax())
    return x0, bank, m_ref, s_ref, x_ref, 0.5 * float(order[i] + order[i + 1])


def test_predict_batch_per_sample_max():
    """predict(per_sample_max=True) at B = 3 with one sample above 1.0 is three B = 1 calls: the same PatchCore input bit
    for bit, scores within REL.  per_sample_max=False halves all three, as the reference's forward would."""
    config = dict(data="mnist")
    for per in (True, False):
        x0, bank, m_ref, s_ref, x_ref, thr = batch_setup(per)
        clf = ldh.PatchCoreClassifier(config, 3, patchcore(84, bank, num_neighbors=1), threshold=thr)
        dec, amap, score = clf.predict(x0.to(DEV), per_sample_max=per)
        x_batch = clf.preprocess(x0.to(DEV), per_sample_max=per).clone()
        assert dec.shape == (3,) and dec.dtype == torch.int32 and amap.shape == (3, 1, 28, 28)
        print(f"batch per_sample_max={per}: pred_score rel err {rel_err(score, s_ref):.2e}, anomaly_map rel err {rel_err(amap, m_ref):.2e}")
        assert rel_err(score, s_ref) < REL and rel_err(amap, m_ref) < REL
        want_dec = (s_ref > thr).to(torch.int32).tolist()
        assert 0 < sum(want_dec) < 3 and dec.tolist() == want_dec
        want64 = cref.preprocess(x0.double(), config, 3, per_sample_max=per)
        assert dist64(x_batch, want64) <= 2 * dist64(x_ref, want64) + FLOOR
        if per:
            for b in range(3):
                assert torch.equal(clf.preprocess(x0[b:b + 1].to(DEV)), x_batch[b:b + 1])
                one = clf.predict(x0[b:b + 1].to(DEV))[2]
                assert rel_err(one, s_ref[b:b + 1]) < REL and rel_err(one, score[b:b + 1].cpu()) < REL
        else:
            halved = cref.preprocess(x0[:1] / 2.0, config, 3)
            assert rel_err(x_batch[:1], halved) < 1e-5


def test_predict_does_not_synchronise():
    """After a warm-up call, predict() runs under set_sync_debug_mode('error'); forward() warns under 'warn' for its one
    .item().  First: the mode is live on this build (a lone .item() under 'warn' warns)."""
    sd, config = state_dict(), dict(data="mnist")
    x0 = gate_input(config, 3, 1, 28, 1, "above", 950)
    with torch.no_grad():
        emb, _ = ref.embedding(ref.features(sd, cref.preprocess(x0, config, 3)))
    clf = ldh.PatchCoreClassifier(config, 3, patchcore(84, planted_bank(emb, 1)[0]), threshold=1.0)
    xd = x0.to(DEV)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            probe.item()
        assert any("synchroniz" in str(i.message).lower() for i in w), "set_sync_debug_mode is not live on this build"
        torch.cuda.set_sync_debug_mode(prev)
        warm = [t.clone() if t is not None else None for t in clf.predict(xd)]
        torch.cuda.set_sync_debug_mode("error")
        dec, amap, score = clf.predict(xd)                               # raises if anything synchronises
        dec_b, _, _ = clf.predict(xd, per_sample_max=True, return_map=False)
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            d, _, _ = clf(xd)
        n_sync = sum("synchroniz" in str(i.message).lower() for i in w)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert n_sync == 1, [str(i.message) for i in w]
    assert d == int(dec.item()) == int(dec_b.item()) == int(warm[0].item())
    assert torch.equal(score, warm[2]) and torch.equal(amap, warm[1])


# ------------------------------------------------------------------------------------------------ calibration
def clean_image(j, H=28):
    return rnd((1, 1, H, H), 901 + 1000 * j, 0.0, 2.0)


def gate_bank(sd, images, config=dict(data="mnist"), obj=3):
    """The embedding rows of clean images pushed through the gate's preprocessing, one call per image."""
    with torch.no_grad():
        return torch.cat([ref.embedding(ref.features(sd, cref.preprocess(im, config, obj)))[0] for im in images])


def calibration_set():
    """12 procedural 28 x 28 images: 6 normal ones (smooth mixtures of the bank's clean images) and 6 with a planted
    far-from-bank region (a saturated square of growing side).  -> (bank, images [12, 1, 28, 28], labels)."""
    sd = state_dict()
    clean = [clean_image(j) for j in range(4)]
    bank = gate_bank(sd, clean)
    images, labels = [], []
    for i in range(6):
        w = 0.15 * (i + 1)
        images.append((1.0 - w) * clean[i % 4] + w * clean[(i + 1) % 4])
        labels.append(0)
    for i in range(6):
        im = ((1.0 - 0.1 * (i + 1)) * clean[i % 4] + 0.1 * (i + 1) * clean[(i + 2) % 4]).clone()
        side = 6 + 3 * i
        im[:, :, 2:2 + side, 3:3 + side] = 2.0 if i % 2 == 0 else 0.0
        images.append(im)
        labels.append(1)
    return bank, torch.cat(images), np.asarray(labels)


def test_calc_threshold_end_to_end():
    """calc_threshold on 12 images = youden_threshold of the CPU reference's scores.  num_neighbors = 1: pred_score is the
    largest patch score, a continuous function of the input, so rounding cannot jump to another support set; and the
    reference scores are more than 10 REL apart, so it cannot reorder them either (asserted before the GPU is used)."""
    sd, config = state_dict(), dict(data="mnist")
    bank, images, labels = calibration_set()
    s_ref = torch.cat([cref.classifier_forward(sd, bank, images[i:i + 1], config, 3, 0.0, num_neighbors=1)[2]
                       for i in range(len(images))]).numpy()
    order = np.sort(s_ref)
    gaps = (order[1:] - order[:-1]) / order[1:]
    print("calibration: reference scores", np.round(s_ref, 3).tolist(), "smallest adjacent gap", f"{gaps.min():.3%}")
    assert gaps.min() > 10 * REL
    want = youden_threshold(s_ref, labels)
    assert np.isfinite(want)                                         # a set with an interior optimum, not the +inf corner
    clf = ldh.PatchCoreClassifier(config, 3, patchcore(84, bank, num_neighbors=1), calibration=(images, labels))
    got_scores = clf.scores(images, batch_size=5)
    print("calibration: HIP scores rel err", f"{np.abs(got_scores - s_ref).max() / s_ref.max():.2e}")
    assert np.abs(got_scores - s_ref).max() / s_ref.max() < REL
    assert np.array_equal(np.argsort(got_scores), np.argsort(s_ref))
    idx = int(np.where(s_ref == np.float32(want))[0][0])             # the threshold IS one image's score
    assert clf.threshold == float(got_scores[idx])
    assert abs(clf.threshold - want) <= REL * s_ref.max()
    assert clf.calc_threshold([images[:7], images[7:]], torch.from_numpy(labels)) == clf.threshold   # any iterable of batches
    dec = clf.predict(images.to(DEV), per_sample_max=True, return_map=False)[0].cpu().numpy()
    assert np.array_equal(dec, (s_ref > want).astype(np.int32))


# ------------------------------------------------------------------------------------------------ the gate in the sampler
def make(kw, config, H, T, final_gain=3.0):
    net = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **kw)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, 0, final_gain=final_gain).items()})
    cfg = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mri", mask_x=False,
               mask_cond=False, ood_AD=False, ood_confidence=False, classifier=False, use_gt=False,
               use_gt_timestep=100)
    cfg.update(config)
    gd = ldh.GaussianDiffusion(cfg, net, image_size=H, timesteps=T, beta_schedule="sigmoid", objective="pred_x0",
                               auto_normalize=False, sampling_timesteps=None).to("cuda")
    gd.noise_source = "host"
    return gd


def run(gd, cond, mask, B):
    out = gd.sample(cond.cuda(), None, batch_size=B, mask=None if mask is None else mask.cuda(), min_max_val=(0.0, 2.0))
    if isinstance(out, list):
        out = torch.stack(out)
    return out.cpu().numpy()


def check(tag, got, want, tol=TOL):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    d = float(np.abs(got - want).max())
    print(f"{tag}: max-abs = {d:.3e}")
    assert d <= tol, (tag, d)


class Recorder:
    """The thin wrapper of the test: keeps a clone of every x0 the gate is handed and of the score it returned."""
    def __init__(self, clf):
        self.clf, self.x0s, self.scores = clf, [], []

    def __call__(self, x0):
        assert x0.is_cuda and x0.dtype == torch.float32 and x0.shape[0] == 1
        self.x0s.append(x0.detach().clone())
        out = self.clf(x0)
        self.scores.append(out[2].clone())
        return out


def oracle_run(unet_sd, unet_cfg, cond, mask, gate, classifier=True):
    o = diffusion_ref.SamplerOptions(timesteps=12, branch_out=True, start_intermediate=True, start_timestep=7, data="mnist",
                                     mask_x=True, classifier=classifier)
    smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(unet_sd, unet_cfg), o, 1, 28)
    smp.classifier = gate
    ns = rng.NoiseStream(10)
    with torch.no_grad():
        out = smp.sample(cond, mask, (0.0, 2.0), 1, lambda s: torch.from_numpy(ns.next(tuple(s))))
    return out.numpy()


def test_gate_drives_the_sampler(golden):
    """test_classifier_gated_rebranching's mnist28 set-up at B = 1 with the real gate instead of a stub.  The threshold is
    chosen on the CPU oracle (all-reject score sequence s_1..s_n, the k with s_(k+1) > max(s_1..s_k) of widest margin, the
    midpoint), and every score the gated oracle run sees is at least 10 REL from it -- asserted before the GPU is used.
    The HIP sampler with PatchCoreClassifier then makes k + 1 calls, each score within REL of classifier_ref on the very
    x0 the gate was handed, and ends within TOL of the oracle.  threshold = -inf accepts at the first call and equals
    the run without the gate.  num_neighbors = 1: with 9 the argmax patch leads by 2e-4 at one call, so the support set
    would not be determinate under a 1e-3 rounding difference (the 9-neighbour score is covered by test_whole_classifier)."""
    g = golden("g9_classifier_gate")
    cond, mask = torch.from_numpy(g["cond28"])[:1], torch.from_numpy(g["mask28"])[:1]
    conf = dict(data="mnist", branch_out=True, start_intermediate=True, start_timestep=7, mask_x=True, classifier=True)
    gd = make(MNIST, conf, 28, 12)
    unet_sd = {k: v.detach().cpu() for k, v in gd.model.state_dict().items()}
    sd, config = state_dict(), dict(data="mnist")
    bank = gate_bank(sd, [torch.from_numpy(rng.uniform((1, 1, 28, 28), 901, j, 0.0, 2.0)) for j in range(3)] + [cond])
    assert bank.shape == (484, 1536)
    # --- the oracle alone
    seq = []
    oracle_run(unet_sd, gd.model.cfg, cond, mask, cref.gate(sd, bank, config, 3, float("inf"), 1, seq))
    print("all-reject score sequence:", np.round(seq, 2).tolist())
    best = None
    for k in range(1, len(seq)):
        top = max(seq[:k])
        if seq[k] > top and (best is None or (seq[k] - top) / (seq[k] + top) > best[1]):
            best = (k, (seq[k] - top) / (seq[k] + top), 0.5 * (seq[k] + top))
    assert best is not None
    k, _, thr = best
    seen = []
    want = oracle_run(unet_sd, gd.model.cfg, cond, mask, cref.gate(sd, bank, config, 3, thr, 1, seen))
    margin = min(abs(s - thr) / thr for s in seen)
    print(f"k = {k}, threshold {thr:.2f}, the gated oracle run makes {len(seen)} calls, margin {margin:.2%}")
    assert len(seen) == k + 1 and seen == seq[:k + 1] and margin >= 10 * REL
    # --- the HIP sampler under the HIP gate
    rec = Recorder(ldh.PatchCoreClassifier(config, 3, patchcore(84, bank, num_neighbors=1), threshold=thr, return_map=False))
    gd.classifier = rec
    got = run(gd, cond, mask, 1)
    assert gd.classifier_calls == k + 1 == len(rec.x0s)
    for i, (x0, s) in enumerate(zip(rec.x0s, rec.scores)):
        s_here = cref.classifier_forward(sd, bank, x0.cpu(), config, 3, thr, num_neighbors=1)[2]
        e, drift = rel_err(s, s_here), abs(float(s[0]) - seen[i]) / seen[i]
        print(f"gate call {i}: score {float(s[0]):.3f}, vs classifier_ref on the same x0 {e:.2e}, vs the oracle's own sequence {drift:.2e}")
        assert e < REL and drift < margin
    check("gated run vs oracle", got, want)
    # --- threshold = -inf: accepted at once, the same as no gate
    gd2 = make(MNIST, conf, 28, 12)
    gd2.classifier = ldh.PatchCoreClassifier(config, 3, rec.clf.patchcore, threshold=float("-inf"))
    got2 = run(gd2, cond, mask, 1)
    assert gd2.classifier_calls == 1
    plain = run(make(MNIST, dict(conf, classifier=False), 28, 12), cond, mask, 1)
    check("threshold -inf vs classifier=False", got2, plain)
    check("classifier=False vs oracle", plain, oracle_run(unet_sd, gd.model.cfg, cond, mask, None, classifier=False))
