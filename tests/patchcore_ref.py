"""Plain-torch restatement of the reference's PatchCore (models.py:42-254 in eval mode, with the anomalib / timm pieces
it imports), the oracle of tests/test_hip_patchcore.py.  Only F.conv2d / F.batch_norm / F.interpolate / F.pad and
tensor ops: no torchvision, no anomalib, no timm.  Inputs are a name-keyed state_dict of the wide_resnet50_2 trunk
(numpy or torch) and fp32 tensors; everything runs on the CPU in fp32."""
import torch
import torch.nn.functional as F

STAGES = (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2))     # blocks, stride of the first block


def _t(sd, k):
    v = sd[k]
    return v if torch.is_tensor(v) else torch.from_numpy(v)


def bn(sd, p, x):
    return F.batch_norm(x, _t(sd, p + "running_mean"), _t(sd, p + "running_var"), _t(sd, p + "weight"), _t(sd, p + "bias"),
                        False, 0.0, 1e-5)


def stem(sd, x):
    """conv1 7x7 s2 p3 -> bn1 -> ReLU (before the max-pool)."""
    return F.relu(bn(sd, "bn1.", F.conv2d(x, _t(sd, "conv1.weight"), stride=2, padding=3)))


def bottleneck(sd, p, x, stride):
    out = F.relu(bn(sd, p + "bn1.", F.conv2d(x, _t(sd, p + "conv1.weight"))))
    out = F.relu(bn(sd, p + "bn2.", F.conv2d(out, _t(sd, p + "conv2.weight"), stride=stride, padding=1)))
    out = bn(sd, p + "bn3.", F.conv2d(out, _t(sd, p + "conv3.weight")))
    if p + "downsample.0.weight" in sd:
        idn = bn(sd, p + "downsample.1.", F.conv2d(x, _t(sd, p + "downsample.0.weight"), stride=stride))
    else:
        idn = x
    return F.relu(out + idn)


def features(sd, x):
    """-> {'layer2': [B, 512, h2, w2], 'layer3': [B, 1024, h3, w3]} (timm features_only, out layers 2 and 3)."""
    x = F.max_pool2d(stem(sd, x), 3, 2, 1)
    feats = {}
    for name, blocks, stride in STAGES:
        for i in range(blocks):
            x = bottleneck(sd, f"{name}.{i}.", x, stride if i == 0 else 1)
        feats[name] = x
    return {"layer2": feats["layer2"], "layer3": feats["layer3"]}


def embedding(feats):
    """AvgPool2d(3, 1, 1) of both maps, bilinear resample of layer3 to the layer2 grid, concat -> [B*h*w, 1536]."""
    l2 = F.avg_pool2d(feats["layer2"], 3, 1, 1)
    l3 = F.avg_pool2d(feats["layer3"], 3, 1, 1)
    l3 = F.interpolate(l3, size=l2.shape[-2:], mode="bilinear", align_corners=False)
    e = torch.cat((l2, l3), 1)
    return e.permute(0, 2, 3, 1).reshape(-1, e.shape[1]), e.shape


def euclidean_dist(x, y):
    x_norm = x.pow(2).sum(dim=-1, keepdim=True)
    y_norm = y.pow(2).sum(dim=-1, keepdim=True)
    res = x_norm - 2 * torch.matmul(x, y.transpose(-2, -1)) + y_norm.transpose(-2, -1)
    return res.clamp_min_(0).sqrt_()


def nearest_neighbors(emb, bank, n):
    d = euclidean_dist(emb, bank)
    if n == 1:
        return d.min(1)
    return d.topk(k=n, largest=False, dim=1)


def anomaly_score(patch_scores, locations, emb, bank, num_neighbors=9):
    if num_neighbors == 1:
        return patch_scores.amax(1)
    B, P = patch_scores.shape
    max_patches = torch.argmax(patch_scores, dim=1)
    feats = emb.reshape(B, P, -1)[torch.arange(B), max_patches]
    score = patch_scores[torch.arange(B), max_patches]
    nn_index = locations[torch.arange(B), max_patches]
    _, support = nearest_neighbors(bank[nn_index, :], bank, min(num_neighbors, bank.shape[0]))
    d = euclidean_dist(feats.unsqueeze(1), bank[support])
    w = (1 - F.softmax(d.squeeze(1), 1))[..., 0]
    return w * score


def gaussian_kernel2d(sigma=4.0):
    ks = 2 * int(4.0 * sigma + 0.5) + 1
    x = torch.arange(ks, dtype=torch.float32) - ks // 2
    g = torch.exp(-x.pow(2.0) / (2 * sigma ** 2))
    g = g / g.sum()
    k2 = g[:, None] * g[None, :]
    return k2 / k2.sum()


def anomaly_map(patch_scores, input_size, sigma=4.0):
    """AnomalyMapGenerator: nearest upsample to input_size, GaussianBlur2d (reflect padding, 2-D conv)."""
    m = F.interpolate(patch_scores, size=tuple(input_size))
    k = gaussian_kernel2d(sigma)
    r = k.shape[0] // 2
    m = F.pad(m, (r, r, r, r), mode="reflect")
    return F.conv2d(m, k[None, None])


def patchcore_forward(sd, bank, x, input_size, num_neighbors=9):
    """-> dict(anomaly_map, pred_score, patch_scores [B, h*w], locations, embedding) of models.py:108-127."""
    with torch.no_grad():
        emb, shape = embedding(features(sd, x))
        B, _, h, w = shape
        ps, loc = nearest_neighbors(emb, bank, 1)
        ps, loc = ps.reshape(B, -1), loc.reshape(B, -1)
        score = anomaly_score(ps, loc, emb, bank, num_neighbors)
        amap = anomaly_map(ps.reshape(B, 1, h, w), input_size)
    return {"anomaly_map": amap, "pred_score": score, "patch_scores": ps, "locations": loc, "embedding": emb}
