"""PatchCore of the reference (``models.PatchcoreModel``, models.py:42-254, eval mode) on the HIP kernels of
``csrc/patchcore.hip``: the default OOD anomaly-map producer that the reference's evaluation runs on the conditioning
image before ``sample(..., mask=...)`` (test.py:150-178, 240-247, ``ood_AD: True`` with ``ood_detector.seg: False``).

``PatchCore`` keeps the ``wide_resnet50_2`` trunk's parameter and buffer names under ``feature_extractor.`` (conv1, bn1,
layer1..3; what anomalib's attribute holds) plus the ``memory_bank`` buffer.  The forward is

* the trunk: the stem (7x7 s2 conv + BatchNorm + ReLU), the 3x3 s2 max-pool and 13 bottlenecks, 42 implicit-GEMM
  convolutions with BatchNorm (eval), the residual and the ReLU in their epilogue;
* the embedding: AvgPool2d(3, 1, 1) of layer2 and layer3, bilinear resample of layer3 to the layer2 grid, concat ->
  [B*h*w, 1536] rows with their squared norms;
* the nearest bank row of every row (fused distance GEMM + min / argmin) -> patch scores;
* the image score of models.py:222-254 (argmax patch, the ``num_neighbors`` bank rows nearest to its neighbour, softmax);
* the anomaly map: nearest upsample to ``input_size`` and the 33x33 Gaussian blur (sigma 4, reflect padding).

All fp32 by default.  ``knn_precision = "fp16"`` runs the nearest-neighbour search of ``nearest`` (and through it
``score``, ``forward`` and the gate) on ``csrc/knn16.hip``: the fp16 matrix cores screen the bank, an fp32 re-rank of the
rows inside a certified window gives the answer, and a query that cannot be certified is searched by the fp32 kernel.
The re-rank sums in the fp32 kernel's own order, so distances and indices are ``"fp32"``'s to the bit (``knn_stats()``
counts the certified and the fallen-back queries).  It keeps an fp16 (hi, lo) copy of the bank beside the fp32 one,
``4 * M * 1536`` bytes more, and refuses a bank with an element beyond fp16's range (``ValueError``).  ``topk`` and the
image score stay fp32.  BatchNorm always uses the running statistics: the module must be in ``eval()`` mode.  No CPU
fallback.
A memory bank is built with ``build_memory_bank`` / ``subsample_embedding`` (anomaly_model_train.py:339-385): the
training embeddings, then anomalib's KCenterGreedy coreset on the kernels of ``csrc/coreset.hip`` (``coreset.py``).
Not covered: other backbones or layers, the tiler, training the trunk.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _cabi as cabi
from .weights import PC_STAGES

BN_EPS = 1e-5
EMBED_DIM = 1536           # 512 (layer2) + 1024 (layer3)
BLUR_SIGMA = 4.0
KNN_PRECISIONS = ("fp32", "fp16")


def gaussian_kernel1d(sigma=BLUR_SIGMA):
    """anomalib's blur kernel, one axis: kornia's Gaussian of size 2 * int(4 sigma + 0.5) + 1, normalised to sum 1
    (fp32).  The 2-D kernel is its outer product, renormalised by its sum."""
    ks = 2 * int(4.0 * sigma + 0.5) + 1
    x = torch.arange(ks, dtype=torch.float32) - ks // 2
    g = torch.exp(-x.pow(2.0) / (2.0 * sigma ** 2))
    return g / g.sum()


def conv_out(n, k, s, p):
    """Output length of a convolution / pooling window: floor((n + 2p - k) / s) + 1."""
    return (n + 2 * p - k) // s + 1


def feature_sizes(h, w):
    """(layer2 grid, layer3 grid) of a h x w input: stem s2, max-pool s2, layer2 s2, layer3 s2."""
    h1, w1 = conv_out(conv_out(h, 7, 2, 3), 3, 2, 1), conv_out(conv_out(w, 7, 2, 3), 3, 2, 1)
    h2, w2 = conv_out(h1, 3, 2, 1), conv_out(w1, 3, 2, 1)
    return (h2, w2), (conv_out(h2, 3, 2, 1), conv_out(w2, 3, 2, 1))


class _Bottleneck(nn.Module):
    def __init__(self, cin, width, cout, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
        else:
            self.downsample = None


class _WideResNet50Trunk(nn.Module):
    """The parameters of ``wide_resnet50_2`` that layers 2 and 3 depend on, under torchvision's / timm's names."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for name, blocks, width, cout, stride in PC_STAGES:
            layer = nn.Sequential(*[_Bottleneck(cin if i == 0 else cout, width, cout, stride if i == 0 else 1, i == 0)
                                    for i in range(blocks)])
            setattr(self, name, layer)
            cin = cout


def _bn_affine(bn):
    """BatchNorm2d (eval) as out = x * s + t, in fp32 from the running statistics."""
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    t = bn.bias.detach().float() - bn.running_mean.detach().float() * s
    return s.contiguous(), t.contiguous()


class PatchCore(nn.Module):
    def __init__(self, input_size, layers=("layer2", "layer3"), backbone="wide_resnet50_2", num_neighbors=9, tiler=None,
                 knn_precision="fp32"):
        super().__init__()
        self._bank16 = None          # (hi, lo, info) of the bank on the device, knn_precision "fp16" only
        self._knn_stats = None       # int32 [4] on the device: certified, fell back, candidate rows, the most per query
        self.knn_precision = knn_precision
        if backbone != "wide_resnet50_2":
            raise ValueError(f"PatchCore: backbone {backbone!r}; only wide_resnet50_2 (test.py:159) has HIP kernels")
        if tuple(layers) != ("layer2", "layer3"):
            raise ValueError(f"PatchCore: layers {tuple(layers)}; only ('layer2', 'layer3') (test.py:161) is supported")
        if tiler is not None:
            raise ValueError("PatchCore: the tiler is not supported")
        if not 1 <= int(num_neighbors) <= 16:
            raise ValueError(f"PatchCore: num_neighbors={num_neighbors} (1..16)")
        self.input_size = (int(input_size[0]), int(input_size[1]))
        self.layers, self.backbone, self.num_neighbors, self.tiler = list(layers), backbone, int(num_neighbors), None
        ks = 2 * int(4.0 * BLUR_SIGMA + 0.5) + 1
        if min(self.input_size) <= ks // 2:
            raise ValueError(f"PatchCore: input_size {self.input_size}: the blur's reflect padding needs more than "
                             f"{ks // 2} pixels per side")
        self.feature_extractor = _WideResNet50Trunk()
        self.register_buffer("memory_bank", torch.empty(0, EMBED_DIM))
        self._prep = None            # device-side weights in kernel layout + BN affines
        self._bank = None            # (bank, norms) on the device
        self._plans = {}             # (B, H, W, device) -> activation buffers

    # ------------------------------------------------------------------ cache control
    @property
    def knn_precision(self):
        """``"fp32"`` (default): ``nearest`` is ``ld_pc_knn``.  ``"fp16"``: ``ld_pc_knn16``, the fp16 screen with the exact
        fp32 re-rank.  Checked on assignment; no part of the ``state_dict``.  Switching to ``"fp16"`` with a bank already
        on the device packs it and raises ``ValueError`` when the bank does not fit fp16's range."""
        return self._knn_precision

    @knn_precision.setter
    def knn_precision(self, value):
        if value not in KNN_PRECISIONS:
            raise ValueError(f"PatchCore: knn_precision {value!r}; one of {KNN_PRECISIONS}")
        old = self.__dict__.get("_knn_precision", "fp32")
        self._knn_precision = value
        bank = self._buffers.get("memory_bank") if "_buffers" in self.__dict__ else None
        if value == "fp16" and bank is not None and bank.is_cuda and bank.numel() > 0:
            try:
                self._bank16_dev(bank.device)
            except ValueError:
                self._knn_precision = old                 # the bank is refused: the mode stays what it was
                raise

    def invalidate(self):
        self._prep = None
        self._bank = None
        self._bank16 = None
        self._plans = {}

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        out = super()._apply(fn, *args, **kwargs)
        if self.knn_precision == "fp16" and self.memory_bank.is_cuda and self.memory_bank.numel() > 0:
            self._bank16_dev(self.memory_bank.device)         # a bank beyond fp16's range is refused when it arrives
        return out

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.invalidate()
        if "memory_bank" in state_dict:                           # any row count: the buffer takes the checkpoint's shape
            self.memory_bank = torch.empty_like(state_dict["memory_bank"], dtype=torch.float32,
                                                device=self.memory_bank.device)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def set_memory_bank(self, bank):
        """The memory bank [M, 1536] (a numpy array or tensor, e.g. ``np.load`` of test.py:169-175); kept as fp32 on the
        module's device.  Its row norms are computed once, on first use."""
        t = torch.as_tensor(np.asarray(bank) if not torch.is_tensor(bank) else bank).to(torch.float32)
        if t.dim() != 2 or t.shape[1] != EMBED_DIM or t.shape[0] < 1:
            raise ValueError(f"PatchCore: memory bank {tuple(t.shape)}, expected [M >= 1, {EMBED_DIM}]")
        self.memory_bank = t.to(self.memory_bank.device).contiguous()
        self._bank = None
        self._bank16 = None
        if self.knn_precision == "fp16" and self.memory_bank.is_cuda:
            self._bank16_dev(self.memory_bank.device)         # ValueError now, not at the first search

    # ------------------------------------------------------------------ weights in kernel layout
    def _prepare(self, dev):
        if self._prep is not None:
            return self._prep
        fe = self.feature_extractor
        with torch.no_grad():
            s, t = _bn_affine(fe.bn1)
            prep = {"stem": (fe.conv1.weight.detach().to(dev, torch.float32).contiguous(), s.to(dev), t.to(dev)),
                    "blocks": []}

            def conv(c, bn):
                w = c.weight.detach().to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()   # OIHW -> OHWI
                s, t = _bn_affine(bn)
                return (w, s.to(dev), t.to(dev), c.weight.shape[1], c.weight.shape[0], c.weight.shape[2])

            for name, blocks, _, _, _ in PC_STAGES:
                for blk in getattr(fe, name):
                    ds = conv(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None
                    prep["blocks"].append((conv(blk.conv1, blk.bn1), conv(blk.conv2, blk.bn2), conv(blk.conv3, blk.bn3),
                                           ds, blk.stride))
            prep["gauss"] = gaussian_kernel1d().to(dev)
        self._prep = prep
        return prep

    def _bank_dev(self, dev):
        if self.memory_bank.numel() == 0:
            raise RuntimeError("PatchCore: the memory bank is empty: set_memory_bank() / load_patchcore() first")
        if self._bank is None:
            bank = self.memory_bank.detach().to(dev, torch.float32).contiguous()
            norms = torch.empty(bank.shape[0], dtype=torch.float32, device=dev)
            cabi.check(cabi.lib().ld_pc_row_norms(bank.data_ptr(), norms.data_ptr(), bank.shape[0], bank.shape[1],
                                                  torch.cuda.current_stream(dev).cuda_stream), "pc_row_norms")
            self._bank = (bank, norms)
        return self._bank

    def _bank16_dev(self, dev):
        """The bank's fp16 split (hi, lo) [M, 1536] and info [2] (largest |m|^2, fp16-finite flag) on the device, packed
        once per bank.  ValueError (one 4-byte read per bank) when an element is beyond fp16's range."""
        if self._bank16 is None:
            bank, bn = self._bank_dev(dev)
            hi = torch.empty(bank.shape, dtype=torch.float16, device=dev)
            lo = torch.empty(bank.shape, dtype=torch.float16, device=dev)
            info = torch.empty(2, dtype=torch.float32, device=dev)
            cabi.check(cabi.lib().ld_pc_pack_bank16(bank.data_ptr(), bn.data_ptr(), bank.shape[0], bank.shape[1],
                                                    hi.data_ptr(), lo.data_ptr(), info.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream), "pc_pack_bank16")
            if float(info[1].item()) != 1.0:
                raise ValueError("PatchCore: knn_precision 'fp16' needs every bank element finite in fp16 "
                                 "(|x| <= 65504); this bank has one that is not: use knn_precision 'fp32'")
            self._bank16 = (hi, lo, info)
        return self._bank16

    def knn_stats(self):
        """(certified, fell back) query counts of the last ``nearest`` at ``knn_precision = "fp16"`` (they sum to its N),
        read from the device on demand; None before the first such search."""
        if self._knn_stats is None:
            return None
        c, f = self._knn_stats.tolist()[:2]
        return int(c), int(f)

    def knn_candidates(self):
        """(bank rows inside all the windows of the last fp16 search together, the most inside one window): what the
        re-rank looked at; a window with more than 64 rows sends its query to the fp32 kernel.  None as ``knn_stats``."""
        if self._knn_stats is None:
            return None
        t, m = self._knn_stats.tolist()[2:]
        return int(t), int(m)

    # ------------------------------------------------------------------ launches
    def _plan(self, B, H, W, dev):
        key = (B, H, W, str(dev))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        prep = self._prepare(dev)
        lib = cabi.lib()
        f32 = dict(dtype=torch.float32, device=dev)
        hs, ws = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
        stem = torch.empty((B, hs, ws, 64), **f32)
        hp, wp = conv_out(hs, 3, 2, 1), conv_out(ws, 3, 2, 1)
        x = torch.empty((B, hp, wp, 64), **f32)
        launches, bufs, feats = [], [stem, x], {}

        def conv(src, layer, h, w, stride, relu=1, residual=None):
            wt, s, t, cin, cout, k = layer
            ho, wo = conv_out(h, k, stride, k // 2), conv_out(w, k, stride, k // 2)
            out = torch.empty((B, ho, wo, cout), **f32)
            bufs.append(out)
            a = cabi.PcConvArgs()
            a.src, a.weight, a.scale, a.shift, a.residual, a.out = (src.data_ptr(), wt.data_ptr(), s.data_ptr(),
                                                                    t.data_ptr(), cabi.ptr(residual), out.data_ptr())
            a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout = B, h, w, cin, ho, wo, cout
            a.ksize, a.stride, a.relu = k, stride, relu
            launches.append(a)
            return out, ho, wo

        h, w = hp, wp
        bi = 0
        for name, blocks, _, _, _ in PC_STAGES:
            for _ in range(blocks):
                c1, c2, c3, ds, stride = prep["blocks"][bi]
                bi += 1
                idn = conv(x, ds, h, w, stride, relu=0)[0] if ds is not None else x
                y, _, _ = conv(x, c1, h, w, 1)
                y, h2, w2 = conv(y, c2, h, w, stride)
                x, h, w = conv(y, c3, h2, w2, 1, relu=1, residual=idn)
            feats[name] = (x, h, w)
        (l2, h2, w2), (l3, h3, w3) = feats["layer2"], feats["layer3"]
        N = B * h2 * w2
        plan = {"stem": stem, "pool": bufs[1], "launches": launches, "bufs": bufs,
                "l2": (l2, h2, w2), "l3": (l3, h3, w3),
                "rows": torch.empty((N, EMBED_DIM), **f32), "norms": torch.empty(N, **f32)}
        self._plans[key] = plan
        return plan

    def _check_input(self, x):
        if self.training:
            raise RuntimeError("PatchCore runs BatchNorm with its running statistics only: call .eval() first "
                               "(test.py:177-178 does)")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"PatchCore: input {tuple(x.shape)}, expected an ImageNet-normalised [B, 3, H, W]")
        B, _, H, W = x.shape
        (h2, w2), (h3, w3) = feature_sizes(H, W)
        if B < 1 or min(h3, w3) < 1 or H < 17 or W < 17:
            raise ValueError(f"PatchCore: input {H}x{W} is too small (at least 17x17)")
        if not torch.cuda.is_available():
            raise RuntimeError("PatchCore needs a GPU (HIP kernels only; there is no CPU fallback)")
        if not x.is_cuda:
            raise ValueError("PatchCore: the input must be a CUDA tensor on the module's device")
        return x.detach().to(torch.float32).contiguous()

    def _features(self, x):
        B, _, H, W = x.shape
        dev = x.device
        plan = self._plan(B, H, W, dev)
        prep = self._prep
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        w0, s0, t0 = prep["stem"]
        stem = plan["stem"]
        cabi.check(lib.ld_pc_stem(x.data_ptr(), w0.data_ptr(), s0.data_ptr(), t0.data_ptr(), stem.data_ptr(), B, H, W, st),
                   "pc_stem")
        pool = plan["pool"]
        cabi.check(lib.ld_pc_maxpool(stem.data_ptr(), pool.data_ptr(), B, stem.shape[1], stem.shape[2], 64, st),
                   "pc_maxpool")
        for a in plan["launches"]:
            cabi.check(lib.ld_pc_conv(C.byref(a), st), "pc_conv")
        (l2, h2, w2), (l3, h3, w3) = plan["l2"], plan["l3"]
        rows, norms = plan["rows"], plan["norms"]
        cabi.check(lib.ld_pc_embed(l2.data_ptr(), l3.data_ptr(), rows.data_ptr(), norms.data_ptr(), B, h2, w2,
                                   l2.shape[-1], h3, w3, l3.shape[-1], st), "pc_embed")
        return rows, norms, (h2, w2)

    # ------------------------------------------------------------------ public
    def embed(self, x):
        """x: ImageNet-normalised NCHW fp32 [B, 3, H, W] on the GPU -> the embedding rows [B*h*w, 1536] in (b, y, x)
        order (the reference's ``training=True`` output; what a memory bank is built from)."""
        x = self._check_input(x)
        rows, _, _ = self._features(x)
        return rows.clone()

    def nearest(self, rows, norms=None):
        """Nearest bank row of each of rows [N, 1536]: (distance [N] fp32, index [N] int64) as
        ``euclidean_dist(rows, memory_bank).min(1)`` (models.py:211-213)."""
        dev = rows.device
        bank, bn = self._bank_dev(dev)
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        rows = rows.detach().to(torch.float32).contiguous()
        N = rows.shape[0]
        if norms is None:
            norms = torch.empty(N, dtype=torch.float32, device=dev)
            cabi.check(lib.ld_pc_row_norms(rows.data_ptr(), norms.data_ptr(), N, EMBED_DIM, st), "pc_row_norms")
        dist = torch.empty(N, dtype=torch.float32, device=dev)
        idx = torch.empty(N, dtype=torch.int32, device=dev)
        if self.knn_precision == "fp16":
            hi, lo, info = self._bank16_dev(dev)
            work = torch.empty(int(lib.ld_pc_knn16_work_bytes(N, EMBED_DIM)), dtype=torch.uint8, device=dev)
            stats = torch.empty(4, dtype=torch.int32, device=dev)
            cabi.check(lib.ld_pc_knn16(rows.data_ptr(), norms.data_ptr(), N, bank.data_ptr(), hi.data_ptr(), lo.data_ptr(),
                                       bn.data_ptr(), info.data_ptr(), bank.shape[0], EMBED_DIM, work.data_ptr(),
                                       dist.data_ptr(), idx.data_ptr(), stats.data_ptr(), st), "pc_knn16")
            self._knn_stats = stats
            return dist, idx
        work = torch.empty(N, dtype=torch.int64, device=dev)
        cabi.check(lib.ld_pc_knn(rows.data_ptr(), norms.data_ptr(), N, bank.data_ptr(), bn.data_ptr(), bank.shape[0],
                                 EMBED_DIM, work.data_ptr(), dist.data_ptr(), idx.data_ptr(), st), "pc_knn")
        return dist, idx

    def topk(self, rows, k, norms=None):
        """The k (<= 16) nearest bank rows of each of rows [N, 1536], ascending: (distances [N, k], indices [N, k] int32)
        as ``topk(k, largest=False)`` (models.py:215), the lower index first on equal distances."""
        dev = rows.device
        bank, bn = self._bank_dev(dev)
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        rows = rows.detach().to(torch.float32).contiguous()
        N = rows.shape[0]
        if norms is None:
            norms = torch.empty(N, dtype=torch.float32, device=dev)
            cabi.check(lib.ld_pc_row_norms(rows.data_ptr(), norms.data_ptr(), N, EMBED_DIM, st), "pc_row_norms")
        d2 = torch.empty((N, bank.shape[0]), dtype=torch.float32, device=dev)
        dist = torch.empty((N, k), dtype=torch.float32, device=dev)
        idx = torch.empty((N, k), dtype=torch.int32, device=dev)
        cabi.check(lib.ld_pc_knn_topk(rows.data_ptr(), norms.data_ptr(), N, bank.data_ptr(), bn.data_ptr(), bank.shape[0],
                                      EMBED_DIM, k, d2.data_ptr(), dist.data_ptr(), idx.data_ptr(), st), "pc_knn_topk")
        return dist, idx

    def score(self, x):
        """The part of ``forward`` in front of the anomaly map: x as there -> (pred_score [B], patch scores [B*h*w],
        (h, w)).  What a caller that only needs the image score launches (the gate of ``classifier.py`` when the map is
        discarded); ``anomaly_map_of`` makes the map from the patch scores."""
        x = self._check_input(x)
        rows, norms, (h, w) = self._features(x)
        B, dev = x.shape[0], x.device
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        bank, bn = self._bank_dev(dev)
        scores, loc = self.nearest(rows, norms)
        P = h * w
        pred = torch.empty(B, dtype=torch.float32, device=dev)
        amax = torch.empty(B, dtype=torch.int32, device=dev)
        k = min(self.num_neighbors, bank.shape[0]) if self.num_neighbors > 1 else 0
        q = torch.empty((B, EMBED_DIM), dtype=torch.float32, device=dev)
        qn = torch.empty(B, dtype=torch.float32, device=dev)
        cabi.check(lib.ld_pc_score_prepare(scores.data_ptr(), loc.data_ptr(), bank.data_ptr(), bn.data_ptr(), B, P,
                                           EMBED_DIM, q.data_ptr(), qn.data_ptr(), amax.data_ptr(), st), "pc_score_prepare")
        support = self.topk(q, k, qn)[1] if k > 0 else None    # k = 0 (num_neighbors == 1): the max patch score
        cabi.check(lib.ld_pc_score(rows.data_ptr(), norms.data_ptr(), scores.data_ptr(), amax.data_ptr(), bank.data_ptr(),
                                   bn.data_ptr(), cabi.ptr(support), B, P, EMBED_DIM, k, pred.data_ptr(), st), "pc_score")
        return pred, scores, (h, w)

    def anomaly_map_of(self, scores, B, h, w):
        """Patch scores [B*h*w] (of ``score``) -> the anomaly map [B, 1, *input_size]."""
        dev = scores.device
        st = torch.cuda.current_stream(dev).cuda_stream
        Ho, Wo = self.input_size
        g = self._prepare(dev)["gauss"]
        tmp = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev)
        amap = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=dev)
        cabi.check(cabi.lib().ld_pc_anomaly_map(scores.data_ptr(), g.data_ptr(), g.numel(), tmp.data_ptr(), amap.data_ptr(),
                                                B, h, w, Ho, Wo, st), "pc_anomaly_map")
        return amap

    def forward(self, x):
        """x: ImageNet-normalised NCHW fp32 [B, 3, H, W] on the GPU -> {"anomaly_map": [B, 1, *input_size],
        "pred_score": [B]} (models.py:108-127)."""
        pred, scores, (h, w) = self.score(x)
        return {"anomaly_map": self.anomaly_map_of(scores, x.shape[0], h, w), "pred_score": pred}

    # ------------------------------------------------------------------ memory-bank construction
    def subsample_embedding(self, embedding, sampling_ratio, **kw):
        """models.py:165-172: the KCenterGreedy coreset of embedding [N, 1536] (on the GPU) becomes the memory bank,
        ``memory_bank = embedding[indices]``.  ``kw`` goes to ``coreset.kcenter_greedy`` (projection, features, start,
        seed).  Returns the indices (int64, pick order).  ValueError when int(N * sampling_ratio) is 0."""
        from .coreset import coreset_size, kcenter_greedy
        if embedding.dim() != 2 or embedding.shape[1] != EMBED_DIM:
            raise ValueError(f"PatchCore: embedding {tuple(embedding.shape)}, expected [N, {EMBED_DIM}]")
        if coreset_size(embedding.shape[0], sampling_ratio) < 1:
            raise ValueError(f"PatchCore: sampling_ratio {sampling_ratio} of {embedding.shape[0]} rows selects none")
        idx = kcenter_greedy(embedding, sampling_ratio=sampling_ratio, **kw)
        self.set_memory_bank(embedding.detach()[idx])
        return idx

    def build_memory_bank(self, batches, sampling_ratio=0.1, **kw):
        """anomaly_model_train.py:348-372: embed every prepared batch (``evalio.patchcore_bank_preprocess``, ImageNet
        normalised [B, 3, H, W]), stack the rows on the device, and ``subsample_embedding`` them.  Returns the indices."""
        dev = self.feature_extractor.conv1.weight.device
        rows = [self.embed(b.to(dev)) for b in batches]
        if not rows:
            raise ValueError("PatchCore.build_memory_bank: no batches")
        return self.subsample_embedding(torch.cat(rows), sampling_ratio, **kw)
