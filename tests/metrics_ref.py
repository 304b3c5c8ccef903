"""References for csrc/metrics.hip (``ld_metric_sums``), all on the CPU:

* ``sums32``: a pure-torch fp32 restatement in the kernel's order -- the horizontal pass, then the vertical one, the eleven
  taps added in index order, every product and sum its own fp32 operation -- with the fp64 sums over windows and elements;
* ``sums64``: the fp64 yardstick, the 11 x 11 window applied with ``F.conv2d`` in double;
* ``direct_ssim_map``: a third, independent statement -- every window written out as a weighted sum in numpy fp64;
* the input builders and the case list of tests/test_hip_metrics.py, and ``D_SSIM`` / ``D_SSE_REL``: the restatement's own
  largest distance from the yardstick over those cases, measured by tests/test_metrics_ref.py (which prints the figures and
  holds the constants to them).  The GPU test's SSIM bound is ``2 * D_SSIM``.

The definition both follow: Wang et al.'s SSIM with the 11-tap Gaussian window (sigma 1.5; taps computed in double,
normalised, rounded to fp32 once), biased moments, K1 = 0.01, K2 = 0.03, no padding (only windows inside the image), a
window belonging to the region of its centre pixel; region 1 = ``mask >= 1``, region 2 = the rest.
"""
import numpy as np
import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng

F32, F64 = torch.float32, torch.float64
WIN, HALF = 11, 5
K1, K2 = 0.01, 0.03

# measured by tests/test_metrics_ref.py::test_measured_distance_of_the_restatement over CASES (the figures it prints),
# rounded up to two digits
D_SSIM = 7.6e-7          # measured 7.595e-07, at (1, 1, 75, 33), L = 1, the one-pixel region (one window per channel)
D_SSE_REL = 0.0          # measured 0: both add the same fp64 squares


def taps64(sigma=1.5):
    d = np.arange(WIN, dtype=np.float64) - HALF
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def taps32(sigma=1.5):
    """The kernel's taps: ``taps64`` rounded to fp32 once."""
    return taps64(sigma).astype(np.float32)


def constants(L):
    return (K1 * float(L)) ** 2, (K2 * float(L)) ** 2


# ------------------------------------------------------------------------------------------------ the SSIM maps
def ssim_map32(x, y, L, sigma=1.5, unbiased=False, pad=False):
    """[B, C, H - 10, W - 10] fp32 in the kernel's order.  The three switches are the mutants of the mutation check: another
    sigma, sample (co)variances (the factor 121 / 120 of the packages' ``use_sample_covariance``), zero-padded borders
    ([B, C, H, W] then)."""
    assert x.dtype == F32 and y.dtype == F32
    if pad:
        x, y = F.pad(x, (HALF,) * 4), F.pad(y, (HALF,) * 4)
    w = torch.from_numpy(taps32(sigma))
    Wo, Ho = x.shape[-1] - (WIN - 1), x.shape[-2] - (WIN - 1)

    def blur(a):
        h = w[0] * a[..., :, 0:Wo]
        for j in range(1, WIN):
            h = h + w[j] * a[..., :, j:j + Wo]
        v = w[0] * h[..., 0:Ho, :]
        for j in range(1, WIN):
            v = v + w[j] * h[..., j:j + Ho, :]
        return v
    mx, my, exx, eyy, exy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    c1, c2 = (torch.tensor(c, dtype=F64).to(F32) for c in constants(L))
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = exx - mxx, eyy - myy, exy - mxy
    if unbiased:
        f = torch.tensor(WIN * WIN / (WIN * WIN - 1.0), dtype=F32)
        sx, sy, sxy = sx * f, sy * f, sxy * f
    return ((2.0 * mxy + c1) * (2.0 * sxy + c2)) / ((mxx + myy + c1) * (sx + sy + c2))


def ssim_map64(x, y, L):
    """The yardstick: the definition in fp64, the 2-D window (outer product of the fp32 taps, widened) through F.conv2d."""
    x, y = x.to(F64), y.to(F64)
    B, C = x.shape[:2]
    t = torch.from_numpy(taps32().astype(np.float64))
    k = torch.outer(t, t)[None, None]

    def blur(a):
        return F.conv2d(a.reshape(B * C, 1, *a.shape[2:]), k).reshape(B, C, a.shape[2] - WIN + 1, a.shape[3] - WIN + 1)
    mx, my = blur(x), blur(y)
    sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    c1, c2 = constants(L)
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))


def direct_ssim_map(x, y, L):
    """[H - 10, W - 10] numpy fp64 for one plane: every window as an explicit weighted sum over its 121 pixels."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = taps32().astype(np.float64)
    k = t[:, None] * t[None, :]
    c1, c2 = constants(L)
    H, W = x.shape
    out = np.zeros((H - WIN + 1, W - WIN + 1))
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            a, b = x[i:i + WIN, j:j + WIN], y[i:i + WIN, j:j + WIN]
            mx, my = (k * a).sum(), (k * b).sum()
            sx, sy, sxy = (k * a * a).sum() - mx * mx, (k * b * b).sum() - my * my, (k * a * b).sum() - mx * my
            out[i, j] = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))
    return out


# ------------------------------------------------------------------------------------------------ the [B, 3, 4] table
def table(pred, ref, mask, ssim, centre_offset=HALF):
    """``ld_metric_sums``'s output from an SSIM map: float64 [B, 3, 4], regions (all, mask >= 1, rest), fields (n_elem, sse,
    n_win, ssim_sum).  ``centre_offset``: where in the image the map's first window has its centre (0 for a padded map)."""
    B, C, H, W = pred.shape
    d = (pred - ref).to(F64)
    sq = d * d
    s = ssim.to(F64)
    Ho, Wo = s.shape[-2:]
    out = torch.zeros(B, 3, 4, dtype=F64)
    regions = [torch.ones(B, 1, H, W, dtype=torch.bool)]
    if mask is not None:
        regions += [mask >= 1.0, ~(mask >= 1.0)]
    for r, m in enumerate(regions):
        mc = m[:, :, centre_offset:centre_offset + Ho, centre_offset:centre_offset + Wo]
        out[:, r, 0] = m.sum(dim=(1, 2, 3)).to(F64) * C
        out[:, r, 1] = (sq * m).sum(dim=(1, 2, 3))
        out[:, r, 2] = mc.sum(dim=(1, 2, 3)).to(F64) * C
        out[:, r, 3] = (s * mc).sum(dim=(1, 2, 3))
    return out


def sums32(pred, ref, mask, L, **mutant):
    return table(pred, ref, mask, ssim_map32(pred, ref, L, **mutant), centre_offset=0 if mutant.get("pad") else HALF)


def sums64(pred, ref, mask, L):
    return table(pred, ref, mask, ssim_map64(pred, ref, L))


def per_image_ssim(t):
    """[B, 3] ssim_sum / n_win of a table (nan for an empty region)."""
    return t[:, :, 3] / t[:, :, 2]


# ------------------------------------------------------------------------------------------------ inputs and cases
SHAPES = [(1, 1, 11, 11),      # one window
          (2, 1, 28, 28),      # MNIST: less than one tile
          (2, 3, 43, 45),      # one and three centres past a tile edge; odd rows: the 16-byte path and its fallback
          (1, 1, 75, 33)]      # three tile rows, one ragged
RANGES = (1.0, 2.0)
MASKS = ("none", "rect", "pixel", "zeros", "ones")


def images(shape, L, seed=0):
    """(pred, ref): two draws of the project's counter generator in [0, L]."""
    key = 1000 * shape[2] + shape[3]
    pred = torch.from_numpy(rng.uniform(shape, seed, 2 * key, 0.0, L))
    ref = torch.from_numpy(rng.uniform(shape, seed, 2 * key + 1, 0.0, L))
    return pred, ref


def make_mask(kind, shape):
    B, _, H, W = shape
    if kind == "none":
        return None
    m = torch.zeros(B, 1, H, W, dtype=F32)
    if kind == "rect":            # cuts the tile edge at 32 + 5 where there is one; other values than 0 / 1 on both sides
        m[:, :, H // 3:H // 3 + max(2, H // 2), W // 4:W // 4 + max(2, W // 2)] = 1.0
        m[:, :, 0, :] = 0.999
        m[:, :, H // 3, W // 4] = 2.5
    elif kind == "pixel":
        m[:, :, H // 2, W // 2] = 1.0
    elif kind == "ones":
        m[:] = 1.0
    else:
        assert kind == "zeros"
    return m


def case_list():
    return [(shape, L, kind) for shape in SHAPES for L in RANGES for kind in MASKS]


def passes(got, want64, d_ssim=None):
    """The comparison of tests/test_hip_metrics.py: counts exact, sse within 1e-12 relative, per-image SSIM of every region
    that has windows within ``2 * D_SSIM`` of the yardstick."""
    d_ssim = D_SSIM if d_ssim is None else d_ssim
    if not (torch.equal(got[:, :, 0], want64[:, :, 0]) and torch.equal(got[:, :, 2], want64[:, :, 2])):
        return False
    if not bool(((got[:, :, 1] - want64[:, :, 1]).abs() <= 1e-12 * want64[:, :, 1]).all()):
        return False
    have = want64[:, :, 2] > 0
    diff = (per_image_ssim(got) - per_image_ssim(want64))[have].abs()
    return bool((diff <= 2.0 * d_ssim).all())
