"""References of the sampler's pointwise kernels (csrc/pointwise.hip, the Fourier time MLP of csrc/time_embed.hip) in pure
torch on the CPU, their input builders and the comparison the GPU tests use.  No device import (as tests/exact_probes.py).

Every reference takes ``dtype``:

* ``torch.float32`` restates the kernel's own operation order.  The library is built with -ffp-contract=off, so + - * /,
  min and max are the same IEEE operations on both sides and the restatement is expected to give the kernel's bits.
* ``torch.float64`` is the yardstick: the same fp32 inputs and fp32 scalars, widened, the same formula.

``make_case`` builds the inputs of one (kernel, shape, variant), evaluates both, and measures ``d`` = the largest
element-wise distance of the fp32 restatement from the fp64 reference, per output.  ``passes`` is the comparison of the
GPU tests: bit equality with the fp32 restatement where the kernel only multiplies by 0 / 1 masks and selects, else
max |got - ref64| <= max(4 d, one fp32 ulp of the largest |ref64|), element-wise, no NaN; the per-sample losses of
p_losses are held to that rule sample by sample (d_b and the ulp of |ref64_b|).  tests/test_pointwise_ref.py
proves the builders' preconditions, pins the references to oracle/diffusion_ref.py and shows that ``passes`` rejects a
set of subtly wrong kernels, all without a GPU.

Draws come from the package's counter generator (rng.uniform, seed 1234, one stream per tensor).
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from localdiffusion_hallucination_amd import rng, schedule

SEED = 1234
T = 50                                   # timesteps of the schedule tables
SHAPES = {
    "SMALL": (3, 3, 7, 9),               # HW = 63: odd, below one workgroup; B = C = 3: both index divisions non-trivial
    "SMALL_C1": (3, 1, 7, 9),
    "LARGE": (2, 3, 419, 419),           # n = 1,053,366 > 4096 * 256: the grid-stride loop makes a second, partial trip
    "PER189": (3, 3, 7, 9),              # q_sample_t / p_losses: fewer elements per sample than threads
    "PER526683": (3, 3, 419, 419),
}
CAP = 4096 * 256                         # elements one trip of the capped grid covers
RANGES = [(0.0, 2.0), (-1.0, 1.0)]
OBJ_NAMES = ("pred_x0", "pred_noise", "pred_v")


def f32(v):
    """A python float that holds an fp32 value (what a ``float`` kernel argument receives)."""
    return float(np.float32(v))


PI32, RSQRT2_32 = f32(math.pi), f32(math.sqrt(0.5))


# ------------------------------------------------------------------------------------------------ input builders
def uni(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, SEED, key, lo, hi))


def values(shape, key, lo, hi):
    """Uniform on [lo, hi) with exact +0.0 at ~4 % and -0.0 at ~4 % of the elements (selectors compare with == 0)."""
    v, u = uni(shape, key, lo, hi), uni(shape, key + 500, 0.0, 1.0)
    v = torch.where(u < 0.04, torch.tensor(0.0), v)
    return torch.where((u >= 0.04) & (u < 0.08), torch.tensor(-0.0), v)


def mask2(B, H, W, key):
    """[B, 1, H, W] with the values 1.0 (35 %), 1.5 (15 %), 0.7 (25 %) and 0.0 (25 %): only >= 1 counts as inside."""
    u = uni((B, 1, H, W), key, 0.0, 1.0)
    m = torch.zeros(B, 1, H, W)
    m[u < 0.75] = 0.7
    m[u < 0.50] = 1.5
    m[u < 0.35] = 1.0
    return m


def masks_k(B, K, H, W, key):
    """[B, K, H, W]: per pixel one owning branch (70 %), none (15 %) or two neighbouring branches (15 %); an owner holds
    1.0 or 1.5, every other branch 0.0 or 0.7."""
    own = (uni((B, H, W), key, 0.0, 1.0) * K).long().clamp(max=K - 1)
    kind = uni((B, H, W), key + 1, 0.0, 1.0)
    k = torch.arange(K)[None, :, None, None]
    inside = (k == own[:, None]) & (kind[:, None] >= 0.15)
    inside |= (k == ((own[:, None] + 1) % K)) & (kind[:, None] >= 0.85)
    u = uni((B, K, H, W), key + 2, 0.0, 1.0)
    return torch.where(inside, torch.where(u < 0.5, 1.0, 1.5), torch.where(u < 0.5, 0.0, 0.7))


def masks_two(mask):
    """The K = 2 masks that reduce the K-mask kernels to the two-branch ones: m_1 = 1 - (m_0 >= 1)."""
    return torch.cat([mask, 1.0 - (mask >= 1.0).float()], dim=1)


@functools.lru_cache(maxsize=None)
def sched_table(objective="pred_x0"):
    """([T, 8] fp32 table in the LD_SCHED_* layout, the buffers it was built from)."""
    buf = schedule.make_buffers(T, "sigmoid", objective)
    table = torch.stack([buf["posterior_mean_coef1"], buf["posterior_mean_coef2"],
                         (0.5 * buf["posterior_log_variance_clipped"]).exp(), buf["sqrt_recip_alphas_cumprod"],
                         buf["sqrt_recipm1_alphas_cumprod"], buf["sqrt_alphas_cumprod"],
                         buf["sqrt_one_minus_alphas_cumprod"], buf["alphas_cumprod"]], 1).contiguous()
    return table, buf


def ddim_scalars(buf, t, t_next, eta):
    """{sr, srm1, sab, s1mab, san, c, sigma, last} of one DDIM pair, fp32 (the reference's fp32 tensor arithmetic)."""
    sr, srm1 = buf["sqrt_recip_alphas_cumprod"][t], buf["sqrt_recipm1_alphas_cumprod"][t]
    sab, s1mab = buf["sqrt_alphas_cumprod"][t], buf["sqrt_one_minus_alphas_cumprod"][t]
    if t_next < 0:
        return [float(sr), float(srm1), float(sab), float(s1mab), 0.0, 0.0, 0.0, 1.0]
    a, an = buf["alphas_cumprod"][t], buf["alphas_cumprod"][t_next]
    sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
    c = (1 - an - sigma ** 2).sqrt()
    return [float(sr), float(srm1), float(sab), float(s1mab), float(an.sqrt()), float(c), float(sigma), 0.0]


@functools.lru_cache(maxsize=None)
def kernel_table(objective="pred_x0"):
    """The table the kernel cases pass: the schedule's, except that row 0 takes row 1's sigma.  The clipped posterior
    variance makes the true sigma_0 1e-10, at which a kernel that wrongly adds the draw at t == 0 could not be told from a
    right one; the kernels do not know where their table comes from."""
    table = sched_table(objective)[0].clone()
    table[0, 2] = table[1, 2]
    return table


@functools.lru_cache(maxsize=None)
def pair_table(steps=5, eta=0.5):
    """[steps, 8] fp32 rows of ld_ddim_step_at for the reference's time pairs; the last row has ``last`` set."""
    _, buf = sched_table()
    _, pairs = schedule.ddim_time_pairs(T, steps)
    return torch.tensor([ddim_scalars(buf, t, tn, eta) for t, tn in pairs], dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ references
def _bin(mask, dtype):
    return (mask >= 1.0).to(dtype)


def _clamp(v, lo, hi):
    return torch.clamp(v, min=lo, max=hi)                    # fminf(fmaxf(v, lo), hi)


def _row(sched, t):
    r = sched.reshape(-1, 8)[0 if t is None else t]
    return [float(v) for v in r]


def _to_x0(x, mo, row, obj):
    if obj == 0:
        return mo
    if obj == 1:
        return row[3] * x - row[4] * mo
    return row[5] * x - row[6] * mo


def ddpm_step(x, mo, z, sched, t, lo, hi, obj, dtype):
    """ld_ddpm_step.  ``t`` None is row mode (``sched`` is the step's row): the draw is added iff there is a noise buffer;
    table mode adds it at t > 0 iff there is one."""
    row = _row(sched, t)
    X = x.to(dtype)
    x0 = _clamp(_to_x0(X, mo.to(dtype), row, obj), lo, hi)
    mean = row[0] * x0 + row[1] * X
    draw = (t is None or t > 0) and z is not None
    return {"x_prev": mean + row[2] * z.to(dtype) if draw else mean, "x0": x0}


def posterior_step(x, x0, z, sched, t, dtype):
    row = _row(sched, t)
    mean = row[0] * x0.to(dtype) + row[1] * x.to(dtype)
    draw = (t is None or t > 0) and z is not None
    return {"x_prev": mean + row[2] * z.to(dtype) if draw else mean}


def ddim_step(x, mo, z, k, lo, hi, obj, dtype):
    """ld_ddim_step; ``k`` = [sr, srm1, sab, s1mab, san, c, sigma, last] (a row of ld_ddim_step_at's pair table)."""
    sr, srm1, sab, s1mab, san, c, sigma, last = k
    X, M = x.to(dtype), mo.to(dtype)
    x0 = M if obj == 0 else (sr * X - srm1 * M if obj == 1 else sab * X - s1mab * M)
    x0 = _clamp(x0, lo, hi)
    if last:
        return {"x_next": x0}
    eps = (sr * X - x0) / srm1
    out = x0 * san + c * eps
    return {"x_next": out + sigma * z.to(dtype) if z is not None else out}


def ddim_step_at(x, mo, z, table, idx, lo, hi, obj, dtype):
    return ddim_step(x, mo, z, [float(v) for v in table[idx]], lo, hi, obj, dtype)


def branch_conditions(cond, mask, lo_clip, dtype):
    b, c = _bin(mask, dtype), cond.to(dtype)
    return {"cond_out": c * b, "cond_in": c * _clamp(1.0 - b, lo_clip, 1.0)}


def branch_conditions_k(cond, masks, lo_clip, dtype):
    """-> [K, B, C, H, W]: branch 0 hard-masked, branches 1.. floored at lo_clip."""
    c = cond.to(dtype)
    outs = []
    for k in range(masks.shape[1]):
        b = _bin(masks[:, k:k + 1], dtype)
        outs.append(c * (b if k == 0 else _clamp(b, lo_clip, 1.0)))
    return {"cond_k": torch.stack(outs)}


def mask_out(mo, mask, min_val, dtype, sel=None):
    b, m = _bin(mask, dtype), mo.to(dtype)
    if sel is not None:
        sel["bin==0"] = (b == 0.0).expand_as(m)
    return {"model_out": torch.where((b == 0.0).expand_as(m), torch.tensor(min_val, dtype=dtype), m * b)}


def fuse_ddpm(xo, xi, x0o, x0i, mask, lo, hi, dtype, sel=None):
    m = _bin(mask, dtype)
    x0 = _clamp(_clamp(x0i.to(dtype), lo, hi) * (1.0 - m) + _clamp(x0o.to(dtype), lo, hi), lo, hi)
    a, c = xo.to(dtype) * m, xi.to(dtype) * (1.0 - m)
    if sel is not None:
        sel["a==0"] = a == 0.0
        sel["a==0 inside"] = (a == 0.0) & (m == 1.0).expand_as(a)
    return {"x": torch.where(a == 0.0, c, a), "x0": x0}


def fuse_ddpm_k(x_first, x_rest, x0_first, x0_rest, masks, lo, hi, dtype, sel=None):
    """x_rest / x0_rest [K-1, B, C, H, W].  x0 = clamp(sum_{k>=1} clamp(x0_k) m_k + clamp(x0_0)); x = first non-zero x_k m_k."""
    K = masks.shape[1]
    m = _bin(masks[:, 1:2], dtype)
    acc = _clamp(x0_rest[0].to(dtype), lo, hi) * m
    a0 = x_first.to(dtype) * _bin(masks[:, 0:1], dtype)
    xv = torch.where(a0 == 0.0, x_rest[0].to(dtype) * m, a0)
    if sel is not None:
        sel["a0==0"] = a0 == 0.0
    for k in range(2, K):
        m = _bin(masks[:, k:k + 1], dtype)
        acc = acc + _clamp(x0_rest[k - 1].to(dtype), lo, hi) * m
        if sel is not None:
            sel[f"xv==0 before {k}"] = xv == 0.0
        xv = torch.where(xv == 0.0, x_rest[k - 1].to(dtype) * m, xv)
    return {"x": xv, "x0": _clamp(acc + _clamp(x0_first.to(dtype), lo, hi), lo, hi)}


def fuse_ddim(xo, xi, x0o, x0i, mask, z, k, lo, hi, dtype, sel=None):
    """ld_fuse_ddim; ``k`` = [sr, srm1, san, c, sigma]."""
    sr, srm1, san, c, sigma = k
    m = _bin(mask, dtype)
    a0, b0 = _clamp(x0o.to(dtype), lo, hi), _clamp(x0i.to(dtype), lo, hi)
    eo, ei = (sr * xo.to(dtype) - a0) / srm1, (sr * xi.to(dtype) - b0) / srm1
    x0 = _clamp(torch.where(a0 == 0.0, b0, a0), lo, hi)
    po, pi = eo * m, ei * (1.0 - m)
    if sel is not None:
        sel["a0==0"], sel["po==0"] = a0 == 0.0, po == 0.0
        sel["po==0 inside"] = (po == 0.0) & (m == 1.0).expand_as(po)
    out = x0 * san + c * torch.where(po == 0.0, pi, po)
    return {"x_next": out + sigma * z.to(dtype) if z is not None else out}


def fuse_ddim_k(x_first, x_rest, x0_first, x0_rest, masks, z, k, lo, hi, dtype, sel=None):
    sr, srm1, san, c, sigma = k
    K = masks.shape[1]
    a0 = _clamp(x0_first.to(dtype), lo, hi)
    eps = (sr * x_first.to(dtype) - a0) / srm1 * _bin(masks[:, 0:1], dtype)
    alt = torch.zeros_like(a0)
    have = torch.zeros_like(a0, dtype=torch.bool)
    for kk in range(1, K):
        m = _bin(masks[:, kk:kk + 1], dtype)
        ak = _clamp(x0_rest[kk - 1].to(dtype), lo, hi)
        ek = (sr * x_rest[kk - 1].to(dtype) - ak) / srm1
        take = ~have & ((m == 1.0) | (kk == K - 1)).expand_as(have)
        alt = torch.where(take, ak, alt)
        have = have | take
        if sel is not None:
            sel[f"eps==0 before {kk}"] = eps == 0.0
            if kk < K - 1:
                sel[f"owner is {kk}"] = take
            elif K > 2:
                sel["no owner: the last branch"] = take & (m != 1.0).expand_as(take)
        eps = torch.where(eps == 0.0, ek * m, eps)
    if sel is not None:
        sel["a0==0"] = a0 == 0.0
    out = _clamp(torch.where(a0 == 0.0, alt, a0), lo, hi) * san + c * eps
    return {"x_next": out + sigma * z.to(dtype) if z is not None else out}


def q_sample(x0, z, sab, s1mab, dtype):
    return {"x": sab * x0.to(dtype) + s1mab * z.to(dtype)}


def q_sample_t(x0, z, t, sab, s1mab, dtype):
    a, c = sab[t].to(dtype).reshape(-1, 1, 1, 1), s1mab[t].to(dtype).reshape(-1, 1, 1, 1)
    return {"x": a * x0.to(dtype) + c * z.to(dtype)}


def p_losses(mo, x0, z, t, sab, s1mab, lw, obj, dtype):
    """ld_p_losses: the squared difference in ``dtype``, its sum over the sample in fp64 (the kernel's accumulator)."""
    a, c = sab[t].to(dtype).reshape(-1, 1, 1, 1), s1mab[t].to(dtype).reshape(-1, 1, 1, 1)
    xs, nz = x0.to(dtype), z.to(dtype)
    target = nz if obj == 1 else (xs if obj == 0 else a * nz - c * xs)
    d = mo.to(dtype) - target
    mean = (d * d).double().reshape(d.shape[0], -1).sum(1) / float(d[0].numel())
    return {"loss": mean.to(dtype) * lw[t].to(dtype)}


def recompose(patches, masks, dtype):
    """patches [B, K, C, H, W], masks [K, H, W] -> sum_k patches_k (m_k >= 1), k ascending."""
    acc = torch.zeros_like(patches[:, 0], dtype=dtype)
    for k in range(masks.shape[0]):
        acc = acc + patches[:, k].to(dtype) * _bin(masks[k], dtype)
    return {"out": acc}


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in fp64, one rounding of the sum to fp64 and one to fp32."""
    return (a.double() * b.double() + c.double()).float()


def time_mlp_fourier(times, weights, w1, b1, w2, b2, dtype):
    """ld_time_mlp_fourier: emb = [t | sin | cos] of the angle ((t w) 2) pi FORMED IN FP32 (the kernel's and the model's
    order) and then widened, Linear, exact GELU, Linear.  fp32: the kernel's ascending fmaf chains from the bias."""
    t = times.float()[:, None]
    ang = (((t * weights[None, :]) * 2.0) * PI32).to(dtype)
    emb = torch.cat([t.to(dtype), torch.sin(ang), torch.cos(ang)], dim=1)

    def linear(v, w, b):
        if dtype == torch.float64:
            return v @ w.double().T + b.double()
        acc = b[None, :].expand(v.shape[0], -1)
        for k in range(w.shape[1]):
            acc = _fma32(w[None, :, k], v[:, k:k + 1], acc)
        return acc
    h = linear(emb, w1, b1)
    h = 0.5 * h * (1.0 + torch.erf(h * RSQRT2_32))
    return {"temb": linear(h, w2, b2)}


# ------------------------------------------------------------------------------------------------ cases
# kernel -> outputs that must equal the fp32 restatement bit for bit (products with 0 / 1 masks and selections only)
EXACT = {"branch_conditions": ("cond_out", "cond_in"), "branch_conditions_k": ("cond_k",), "mask_out": ("model_out",),
         "fuse_ddpm": ("x",), "fuse_ddpm_k": ("x",)}
# kernel -> outputs held to the bound sample by sample: the losses of t = T - 1 and t = 0 lie seven decades apart
EACH = {"p_losses": ("loss",)}
DDPM_MODES = ("t0", "t1", "tlast", "row_z", "row_noz", "t1_noz")
_MODE_T = {"t0": 0, "t1": 1, "tlast": T - 1, "row_z": None, "row_noz": None, "t1_noz": 1}
ROW_T = 17                               # the timestep whose row the row-mode cases pass


def _branch_inputs(shape, lo, hi, key, K=None):
    """States in a range wider than (lo, hi) with planted zeros; predictions that reach below lo and above hi."""
    B, C, H, W = shape
    s = (B, C, H, W)
    r = s if K is None else (K - 1,) + s
    xa, xb, pa, pb = values(s, key, -2, 2), values(r, key + 1, -2, 2), values(s, key + 2, lo - 1, hi + 1), values(r, key + 3, lo - 1, hi + 1)
    # a state AND its prediction exactly zero at ~6 % of the elements: the one way eps = (sr x - x0) / srm1 is exactly zero
    for x, p, k in ((xa, pa, key + 5), (xb, pb, key + 6)):
        both = uni(x.shape, k, 0.0, 1.0) < 0.06
        x[both], p[both] = 0.0, 0.0
    if K is None:
        return NS(xo=xa, xi=xb, x0o=pa, x0i=pb, mask=mask2(B, H, W, key + 4))
    return NS(x_first=xa, x_rest=xb, x0_first=pa, x0_rest=pb, masks=masks_k(B, K, H, W, key + 4))


def _fuse_scalars(row=1):
    r = [float(v) for v in pair_table()[row]]
    return [r[0], r[1], r[4], r[5], r[6]]


def build(kernel, shape, v):
    """-> (inputs, ref) with ref(inputs, dtype, sel=None) -> {output name: tensor}."""
    B, C, H, W = shape
    s = (B, C, H, W)
    lo, hi = v.get("lohi", RANGES[0])
    obj = v.get("obj", 0)
    table = kernel_table(OBJ_NAMES[obj])
    if kernel in ("ddpm_step", "posterior_step"):
        t = _MODE_T[v["mode"]]
        sched = table if t is not None else table[ROW_T:ROW_T + 1].clone()
        z = None if v["mode"].endswith("noz") else uni(s, 12, -2, 2)
        if kernel == "ddpm_step":
            i = NS(x=values(s, 10, -2, 2), mo=values(s, 11, lo - 1, hi + 1), z=z, sched=sched, t=t, lo=lo, hi=hi, obj=obj)
            return i, lambda i, dt, sel=None: ddpm_step(i.x, i.mo, i.z, i.sched, i.t, i.lo, i.hi, i.obj, dt)
        i = NS(x=values(s, 10, -2, 2), x0=values(s, 13, lo, hi), z=z, sched=sched, t=t)
        return i, lambda i, dt, sel=None: posterior_step(i.x, i.x0, i.z, i.sched, i.t, dt)
    if kernel == "ddim_step":
        idx = {"plain": 1, "noz": 2, "last": pair_table().shape[0] - 1}[v["variant"]]
        z = None if v["variant"] == "noz" else uni(s, 22, -2, 2)
        i = NS(x=values(s, 20, -2, 2), mo=values(s, 21, lo - 1, hi + 1), z=z, table=pair_table(), idx=idx, lo=lo, hi=hi, obj=obj)
        return i, lambda i, dt, sel=None: ddim_step_at(i.x, i.mo, i.z, i.table, i.idx, i.lo, i.hi, i.obj, dt)
    if kernel == "branch_conditions":
        i = NS(cond=values(s, 30, 0, 2), mask=mask2(B, H, W, 31), lo_clip=v["lo_clip"])
        return i, lambda i, dt, sel=None: branch_conditions(i.cond, i.mask, i.lo_clip, dt)
    if kernel == "branch_conditions_k":
        i = NS(cond=values(s, 32, 0, 2), masks=masks_k(B, v["K"], H, W, 33), lo_clip=v["lo_clip"])
        return i, lambda i, dt, sel=None: branch_conditions_k(i.cond, i.masks, i.lo_clip, dt)
    if kernel == "mask_out":
        i = NS(mo=values(s, 34, lo - 1, hi + 1), mask=mask2(B, H, W, 35), min_val=lo)
        return i, lambda i, dt, sel=None: mask_out(i.mo, i.mask, i.min_val, dt, sel)
    if kernel == "fuse_ddpm":
        i = _branch_inputs(shape, lo, hi, 40)
        i.lo, i.hi = lo, hi
        return i, lambda i, dt, sel=None: fuse_ddpm(i.xo, i.xi, i.x0o, i.x0i, i.mask, i.lo, i.hi, dt, sel)
    if kernel == "fuse_ddpm_k":
        i = _branch_inputs(shape, lo, hi, 50, v["K"])
        i.lo, i.hi = lo, hi
        return i, lambda i, dt, sel=None: fuse_ddpm_k(i.x_first, i.x_rest, i.x0_first, i.x0_rest, i.masks, i.lo, i.hi, dt, sel)
    if kernel in ("fuse_ddim", "fuse_ddim_k"):
        K = v.get("K")
        i = _branch_inputs(shape, lo, hi, 60 if K is None else 70, K)
        i.lo, i.hi, i.k = lo, hi, _fuse_scalars()
        i.z = None if v.get("noz") else uni(s, 65, -2, 2)
        if K is None:
            return i, lambda i, dt, sel=None: fuse_ddim(i.xo, i.xi, i.x0o, i.x0i, i.mask, i.z, i.k, i.lo, i.hi, dt, sel)
        return i, lambda i, dt, sel=None: fuse_ddim_k(i.x_first, i.x_rest, i.x0_first, i.x0_rest, i.masks, i.z, i.k, i.lo, i.hi, dt, sel)
    buf = sched_table(OBJ_NAMES[obj])[1]
    if kernel == "q_sample":
        i = NS(x0=values(s, 80, lo, hi), z=uni(s, 81, -3, 3), sab=float(buf["sqrt_alphas_cumprod"][ROW_T]),
               s1mab=float(buf["sqrt_one_minus_alphas_cumprod"][ROW_T]))
        return i, lambda i, dt, sel=None: q_sample(i.x0, i.z, i.sab, i.s1mab, dt)
    if kernel in ("q_sample_t", "p_losses"):
        t = torch.tensor([T - 1, 0, ROW_T][:B] + [5] * max(0, B - 3))
        i = NS(mo=values(s, 82, lo - 1, hi + 1), x0=values(s, 83, lo, hi), z=uni(s, 84, -3, 3), t=t, sab=buf["sqrt_alphas_cumprod"],
               s1mab=buf["sqrt_one_minus_alphas_cumprod"], lw=buf["loss_weight"], obj=obj)
        if kernel == "q_sample_t":
            return i, lambda i, dt, sel=None: q_sample_t(i.x0, i.z, i.t, i.sab, i.s1mab, dt)
        return i, lambda i, dt, sel=None: p_losses(i.mo, i.x0, i.z, i.t, i.sab, i.s1mab, i.lw, i.obj, dt)
    if kernel == "recompose":
        K = v["K"]
        i = NS(patches=values((B, K, C, H, W), 90, -2, 2), masks=masks_k(1, K, H, W, 91)[0])
        return i, lambda i, dt, sel=None: recompose(i.patches, i.masks, dt)
    if kernel == "time_mlp_fourier":
        ld, td = v["learned_dim"], v["time_dim"]
        i = NS(times=torch.tensor([0, 1, 500, 999], dtype=torch.int32), weights=uni((ld // 2,), 100, -1.5, 1.5),
               w1=uni((td, ld + 1), 101, -0.1, 0.1), b1=uni((td,), 102), w2=uni((td, td), 103, -0.1, 0.1), b2=uni((td,), 104))
        # |t| reaches 999 in emb[0]: scale its column down as a trained layer would
        i.w1[:, 0] *= 1e-3
        return i, lambda i, dt, sel=None: time_mlp_fourier(i.times, i.weights, i.w1, i.b1, i.w2, i.b2, dt)
    raise KeyError(kernel)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def bound(ref64, d):
    """max(4 d, one fp32 ulp of the largest |ref64|): 4 is the project's convention (tests/test_hip_segtrain.py); it leaves
    room for another association and the device's division and transcendental rounding."""
    return max(4.0 * d, ulp32(float(ref64.abs().max())))


def make_case(kernel, shape_name, **v):
    return _make_case(kernel, shape_name, tuple(sorted(v.items())))


@functools.lru_cache(maxsize=4)           # (a LARGE case holds ~100 MB: shared by neighbouring tests, not kept for the session)
def _make_case(kernel, shape_name, items):
    v = dict(items)
    inp, ref = build(kernel, SHAPES[shape_name], v)
    sel32, sel64 = {}, {}
    ref32, ref64 = ref(inp, torch.float32, sel32), ref(inp, torch.float64, sel64)
    d, d_each = {}, {}
    for name in ref64:
        assert ref32[name].dtype == torch.float32 and ref64[name].dtype == torch.float64, (kernel, name)
        assert bool(torch.isfinite(ref64[name]).all()), (kernel, name)
        d_each[name] = (ref32[name].double() - ref64[name]).abs()
        d[name] = float(d_each[name].max())
    return NS(kernel=kernel, shape=SHAPES[shape_name], shape_name=shape_name, v=v, inp=inp, ref=ref, ref32=ref32, ref64=ref64,
              d=d, d_each=d_each, sel32=sel32, sel64=sel64, exact=EXACT.get(kernel, ()), each=EACH.get(kernel, ()))


def bound_each(ref64, d_each):
    """bound() of every element by itself: max(4 d_b, one fp32 ulp of |ref64_b|), as an fp64 tensor."""
    ulp = torch.from_numpy(np.spacing(ref64.abs().float().numpy())).double()
    return torch.maximum(4.0 * d_each, ulp)


def errors(case, got):
    """{output: (passes, max error or None for the bit comparison, bound)} of a kernel's outputs (fp32 cpu tensors).  An
    output in EACH (one value per sample, of very different sizes) reports the error and the bound of its worst sample."""
    res = {}
    for name, ref64 in case.ref64.items():
        g = got[name]
        assert g.shape == ref64.shape and g.dtype == torch.float32, (name, g.shape, ref64.shape, g.dtype)
        if name in case.exact:
            res[name] = (torch.equal(g, case.ref32[name]), None, 0.0)
            continue
        err = (g.double() - ref64).abs()                              # NaN where an element is
        if name in case.each:
            bnd = bound_each(ref64, case.d_each[name])
            ok = bool(torch.isfinite(g).all()) and bool((err <= bnd).all())
            worst = int(torch.nan_to_num(err / bnd, nan=float("inf")).argmax())
            res[name] = (ok, float(err.reshape(-1)[worst]), float(bnd.reshape(-1)[worst]))
            continue
        bnd, err = bound(ref64, case.d[name]), float(err.max())
        res[name] = (bool(torch.isfinite(g).all()) and err <= bnd, err, bnd)
    return res


def passes(case, got):
    return all(ok for ok, _, _ in errors(case, got).values())


def case_list():
    """[(kernel, shape name, variant)]: every kernel at both sizes, the K-mask kernels with K in {2, 3, 5} at SMALL and
    K = 3 at LARGE; every variant at the small shapes, one per code path at LARGE."""
    out = []
    small = ("SMALL", "SMALL_C1")
    for sn in small:
        for lohi in RANGES:
            for obj in range(3):
                out += [("ddpm_step", sn, dict(mode=m, obj=obj, lohi=lohi)) for m in DDPM_MODES]
                out += [("ddim_step", sn, dict(variant=vv, obj=obj, lohi=lohi)) for vv in ("plain", "noz", "last")]
            out += [("posterior_step", sn, dict(mode=m, lohi=lohi)) for m in DDPM_MODES]
            out += [("mask_out", sn, dict(lohi=lohi)), ("fuse_ddpm", sn, dict(lohi=lohi)), ("q_sample", sn, dict(lohi=lohi))]
            out += [("fuse_ddim", sn, dict(lohi=lohi, noz=nz)) for nz in (False, True)]
            for K in (2, 3, 5):
                out += [("fuse_ddpm_k", sn, dict(K=K, lohi=lohi)), ("fuse_ddim_k", sn, dict(K=K, lohi=lohi, noz=False))]
            out.append(("fuse_ddim_k", sn, dict(K=3, lohi=lohi, noz=True)))
        for lc in (0.95, 0.5):
            out.append(("branch_conditions", sn, dict(lo_clip=f32(lc))))
            out += [("branch_conditions_k", sn, dict(K=K, lo_clip=f32(lc))) for K in (2, 3, 5)]
        out.append(("recompose", sn, dict(K=4)))
    sn = "LARGE"
    for obj in range(3):
        out += [("ddpm_step", sn, dict(mode="t1", obj=obj, lohi=RANGES[0])), ("ddim_step", sn, dict(variant="plain", obj=obj, lohi=RANGES[1]))]
    out += [("ddpm_step", sn, dict(mode="row_z", obj=1, lohi=RANGES[1])), ("ddpm_step", sn, dict(mode="t0", obj=0, lohi=RANGES[0])),
            ("ddim_step", sn, dict(variant="last", obj=2, lohi=RANGES[0])), ("ddim_step", sn, dict(variant="noz", obj=0, lohi=RANGES[0])),
            ("posterior_step", sn, dict(mode="t1", lohi=RANGES[0])), ("posterior_step", sn, dict(mode="row_noz", lohi=RANGES[1])),
            ("branch_conditions", sn, dict(lo_clip=f32(0.95))), ("branch_conditions_k", sn, dict(K=3, lo_clip=f32(0.95))),
            ("recompose", sn, dict(K=4))]
    for lohi in RANGES:
        out += [("mask_out", sn, dict(lohi=lohi)), ("fuse_ddpm", sn, dict(lohi=lohi)), ("fuse_ddpm_k", sn, dict(K=3, lohi=lohi)),
                ("fuse_ddim", sn, dict(lohi=lohi, noz=False)), ("fuse_ddim_k", sn, dict(K=3, lohi=lohi, noz=False)),
                ("q_sample", sn, dict(lohi=lohi))]
    for sn in ("PER189", "PER526683"):
        out.append(("q_sample_t", sn, dict(lohi=RANGES[0])))
        out += [("p_losses", sn, dict(obj=obj, lohi=RANGES[obj % 2])) for obj in range(3)]
    for ld in (2, 16):
        out += [("time_mlp_fourier", "SMALL", dict(learned_dim=ld, time_dim=td)) for td in (64, 128)]
    return out


def case_id(c):
    kernel, sn, v = c
    return "-".join([kernel, sn] + [f"{k}{'_'.join(str(x) for x in val) if isinstance(val, tuple) else val}" for k, val in sorted(v.items())])
