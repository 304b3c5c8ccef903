"""The sampler's pointwise kernels (csrc/pointwise.hip), the head-of-step work (step_begin_work in common.hip.h, alone and
inside the stem convolution) and the Fourier time MLP, each called directly and compared ELEMENT-WISE with the references
of tests/pointwise_ref.py: bit equality with the fp32 restatement where a kernel only multiplies by 0 / 1 masks and
selects, else max |got - ref64| <= max(4 d, one fp32 ulp of max |ref64|) with d the restatement's own measured error
(the per-sample losses of ld_p_losses: that rule sample by sample, each against its own d_b and ulp).
tests/test_pointwise_ref.py shows on the CPU that this comparison rejects a set of subtly wrong kernels.  Shapes are the
smallest at which the code can go wrong (HW = 63 below one workgroup, n just above the 4096-block cap), not the
workload's.  Every output buffer holds NaN before the launch.  ``-s`` prints d, the observed error and their ratio."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
import hip_helpers as hh                                           # noqa: E402
import pointwise_ref as R                                          # noqa: E402

DTYPES = ["fp32", "bf16", "fp16"]
LOWP = ["bf16", "fp16"]
LD_EINVAL = -1


def dev(t):
    return None if t is None else t.contiguous().to(hh.DEV)


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=hh.DEV)


def P(t):
    return cabi.ptr(t)


def dims(t):
    B, Cc, H, W = t.shape[-4:]
    return B, Cc, H * W


# ------------------------------------------------------------------------------------------------ launches
def run_ddpm_step(i, x0_out=True, inplace=False):
    x, mo, z, sched = dev(i.x), dev(i.mo), dev(i.z), dev(i.sched)
    tdev = None if i.t is None else i32(i.t)
    xp = x if inplace else torch.full_like(x, hh.NAN)
    x0o = torch.full_like(x, hh.NAN) if x0_out else None
    cabi.check(cabi.lib().ld_ddpm_step(x.data_ptr(), mo.data_ptr(), P(z), xp.data_ptr(), P(x0o), sched.data_ptr(), P(tdev),
                                       i.lo, i.hi, i.obj, x.numel(), hh.st()), "ddpm_step")
    return {"x_prev": xp.cpu(), "x0": None if x0o is None else x0o.cpu()}


def run_posterior_step(i, inplace=False):
    x, x0, z, sched = dev(i.x), dev(i.x0), dev(i.z), dev(i.sched)
    tdev = None if i.t is None else i32(i.t)
    xp = x if inplace else torch.full_like(x, hh.NAN)
    cabi.check(cabi.lib().ld_posterior_step(x.data_ptr(), x0.data_ptr(), P(z), xp.data_ptr(), sched.data_ptr(), P(tdev),
                                            x.numel(), hh.st()), "posterior_step")
    return {"x_prev": xp.cpu()}


def run_ddim_step(i):
    """ld_ddim_step with the row's scalars and ld_ddim_step_at selecting the row through the device index: the same bits."""
    lib = cabi.lib()
    x, mo, z, table = dev(i.x), dev(i.mo), dev(i.z), dev(i.table)
    a, b = torch.full_like(x, hh.NAN), torch.full_like(x, hh.NAN)
    r = [float(v) for v in i.table[i.idx]]
    cabi.check(lib.ld_ddim_step(x.data_ptr(), mo.data_ptr(), P(z), a.data_ptr(), r[0], r[1], r[2], r[3], r[4], r[5], r[6],
                                i.lo, i.hi, i.obj, int(r[7]), x.numel(), hh.st()), "ddim_step")
    cabi.check(lib.ld_ddim_step_at(x.data_ptr(), mo.data_ptr(), P(z), b.data_ptr(), table.data_ptr(), i32(i.idx).data_ptr(),
                                   i.lo, i.hi, i.obj, x.numel(), hh.st()), "ddim_step_at")
    assert torch.equal(a, b)
    return {"x_next": b.cpu()}


def run_branch_conditions(i):
    cond, mask = dev(i.cond), dev(i.mask)
    B, Cc, HW = dims(cond)
    co, ci = torch.full_like(cond, hh.NAN), torch.full_like(cond, hh.NAN)
    cabi.check(cabi.lib().ld_branch_conditions(cond.data_ptr(), mask.data_ptr(), co.data_ptr(), ci.data_ptr(), i.lo_clip,
                                               B, Cc, HW, hh.st()), "branch_conditions")
    return {"cond_out": co.cpu(), "cond_in": ci.cpu()}


def run_branch_conditions_k(i):
    cond, masks = dev(i.cond), dev(i.masks)
    B, Cc, HW = dims(cond)
    K = masks.shape[1]
    out = hh.nans(K, *cond.shape)
    cabi.check(cabi.lib().ld_branch_conditions_k(cond.data_ptr(), masks.data_ptr(), out.data_ptr(), i.lo_clip, B, Cc, K, HW,
                                                 hh.st()), "branch_conditions_k")
    return {"cond_k": out.cpu()}


def run_mask_out(i):
    mo, mask = dev(i.mo).clone(), dev(i.mask)
    B, Cc, HW = dims(mo)
    cabi.check(cabi.lib().ld_mask_out(mo.data_ptr(), mask.data_ptr(), i.min_val, B, Cc, HW, hh.st()), "mask_out")
    return {"model_out": mo.cpu()}


def run_fuse_ddpm(i):
    xo, xi, x0o, x0i, mask = [dev(t) for t in (i.xo, i.xi, i.x0o, i.x0i, i.mask)]
    B, Cc, HW = dims(xo)
    x, x0 = torch.full_like(xo, hh.NAN), torch.full_like(xo, hh.NAN)
    cabi.check(cabi.lib().ld_fuse_ddpm(xo.data_ptr(), xi.data_ptr(), x0o.data_ptr(), x0i.data_ptr(), mask.data_ptr(),
                                       x.data_ptr(), x0.data_ptr(), i.lo, i.hi, B, Cc, HW, hh.st()), "fuse_ddpm")
    return {"x": x.cpu(), "x0": x0.cpu()}


def run_fuse_ddpm_k(i):
    xf, xr, pf, pr, masks = [dev(t) for t in (i.x_first, i.x_rest, i.x0_first, i.x0_rest, i.masks)]
    B, Cc, HW = dims(xf)
    assert xr.shape == (masks.shape[1] - 1,) + xf.shape == pr.shape and masks.shape[0] == B
    x, x0 = torch.full_like(xf, hh.NAN), torch.full_like(xf, hh.NAN)
    cabi.check(cabi.lib().ld_fuse_ddpm_k(xf.data_ptr(), xr.data_ptr(), pf.data_ptr(), pr.data_ptr(), masks.data_ptr(),
                                         x.data_ptr(), x0.data_ptr(), i.lo, i.hi, B, Cc, masks.shape[1], HW, hh.st()), "fuse_ddpm_k")
    return {"x": x.cpu(), "x0": x0.cpu()}


def run_fuse_ddim(i):
    xo, xi, x0o, x0i, mask, z = [dev(t) for t in (i.xo, i.xi, i.x0o, i.x0i, i.mask, i.z)]
    B, Cc, HW = dims(xo)
    xn = torch.full_like(xo, hh.NAN)
    sr, srm1, san, c, sigma = i.k
    cabi.check(cabi.lib().ld_fuse_ddim(xo.data_ptr(), xi.data_ptr(), x0o.data_ptr(), x0i.data_ptr(), mask.data_ptr(), P(z),
                                       xn.data_ptr(), sr, srm1, san, c, sigma, i.lo, i.hi, B, Cc, HW, hh.st()), "fuse_ddim")
    return {"x_next": xn.cpu()}


def run_fuse_ddim_k(i):
    xf, xr, pf, pr, masks, z = [dev(t) for t in (i.x_first, i.x_rest, i.x0_first, i.x0_rest, i.masks, i.z)]
    B, Cc, HW = dims(xf)
    assert xr.shape == (masks.shape[1] - 1,) + xf.shape == pr.shape and masks.shape[0] == B
    xn = torch.full_like(xf, hh.NAN)
    sr, srm1, san, c, sigma = i.k
    cabi.check(cabi.lib().ld_fuse_ddim_k(xf.data_ptr(), xr.data_ptr(), pf.data_ptr(), pr.data_ptr(), masks.data_ptr(), P(z),
                                         xn.data_ptr(), sr, srm1, san, c, sigma, i.lo, i.hi, B, Cc, masks.shape[1], HW,
                                         hh.st()), "fuse_ddim_k")
    return {"x_next": xn.cpu()}


def run_q_sample(i):
    x0, z = dev(i.x0), dev(i.z)
    out = torch.full_like(x0, hh.NAN)
    cabi.check(cabi.lib().ld_q_sample(x0.data_ptr(), z.data_ptr(), out.data_ptr(), i.sab, i.s1mab, x0.numel(), hh.st()), "q_sample")
    return {"x": out.cpu()}


def run_q_sample_t(i):
    x0, z, sab, s1mab = dev(i.x0), dev(i.z), dev(i.sab), dev(i.s1mab)
    t = i.t.to(hh.DEV, torch.int32)
    out = torch.full_like(x0, hh.NAN)
    cabi.check(cabi.lib().ld_q_sample_t(x0.data_ptr(), z.data_ptr(), out.data_ptr(), t.data_ptr(), sab.data_ptr(), s1mab.data_ptr(),
                                        x0.shape[0], x0[0].numel(), hh.st()), "q_sample_t")
    return {"x": out.cpu()}


def run_p_losses(i):
    mo, x0, z, sab, s1mab, lw = [dev(t) for t in (i.mo, i.x0, i.z, i.sab, i.s1mab, i.lw)]
    t = i.t.to(hh.DEV, torch.int32)
    loss = hh.nans(x0.shape[0])
    cabi.check(cabi.lib().ld_p_losses(mo.data_ptr(), x0.data_ptr(), z.data_ptr(), t.data_ptr(), sab.data_ptr(), s1mab.data_ptr(),
                                      lw.data_ptr(), loss.data_ptr(), x0.shape[0], x0[0].numel(), i.obj, hh.st()), "p_losses")
    return {"loss": loss.cpu()}


def run_recompose(i):
    patches, masks = dev(i.patches), dev(i.masks)
    B, K, Cc, H, W = patches.shape
    out = hh.nans(B, Cc, H, W)
    cabi.check(cabi.lib().ld_recompose(patches.data_ptr(), masks.data_ptr(), out.data_ptr(), B, K, Cc, H * W, hh.st()), "recompose")
    return {"out": out.cpu()}


def run_time_mlp_fourier(i):
    times, weights, w1, b1, w2, b2 = [dev(t) for t in (i.times, i.weights, i.w1, i.b1, i.w2, i.b2)]
    td = w2.shape[0]
    temb = hh.nans(times.numel(), td)
    cabi.check(cabi.lib().ld_time_mlp_fourier(times.data_ptr(), times.numel(), weights.data_ptr(), 2 * weights.numel(),
                                              w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), td, temb.data_ptr(),
                                              hh.st()), "time_mlp_fourier")
    return {"temb": temb.cpu()}


RUN = {"ddpm_step": run_ddpm_step, "posterior_step": run_posterior_step, "ddim_step": run_ddim_step,
       "branch_conditions": run_branch_conditions, "branch_conditions_k": run_branch_conditions_k, "mask_out": run_mask_out,
       "fuse_ddpm": run_fuse_ddpm, "fuse_ddpm_k": run_fuse_ddpm_k, "fuse_ddim": run_fuse_ddim, "fuse_ddim_k": run_fuse_ddim_k,
       "q_sample": run_q_sample, "q_sample_t": run_q_sample_t, "p_losses": run_p_losses, "recompose": run_recompose,
       "time_mlp_fourier": run_time_mlp_fourier}


def check(case, got, what):
    res = R.errors(case, got)
    for name, (ok, err, bnd) in res.items():
        d = case.d[name]
        if err is None:
            print(f"RECORD {what} {name}: bit-equal to the fp32 restatement: {ok}")
        elif name in case.each:                      # the bound holds sample by sample
            e, b = (got[name].double() - case.ref64[name]).abs(), R.bound_each(case.ref64[name], case.d_each[name])
            for k in range(e.numel()):
                print(f"RECORD {what} {name}[{k}]: ref {float(case.ref64[name][k]):.6e} d {float(case.d_each[name][k]):.3e} "
                      f"gpu {float(e[k]):.3e} bound {float(b[k]):.3e} bit-equal {bool(got[name][k] == case.ref32[name][k])}")
        else:
            print(f"RECORD {what} {name}: d {d:.3e} gpu {err:.3e} ratio {err / d if d else float('inf') if err else 0.0:.2f} bound {bnd:.3e} "
                  f"bit-equal {torch.equal(got[name], case.ref32[name])}")
    assert all(ok for ok, _, _ in res.values()), res


@pytest.mark.parametrize("c", R.case_list(), ids=R.case_id)
def test_kernel(c):
    kernel, sn, v = c
    case = R.make_case(kernel, sn, **v)
    check(case, RUN[kernel](case.inp), R.case_id(c))


# ------------------------------------------------------------------------------------------------ beyond the plain call
@pytest.mark.parametrize("sn", ["SMALL", "LARGE"])
@pytest.mark.parametrize("mode", ["t1", "t0", "row_z", "t1_noz"])
def test_ddpm_step_in_place_and_without_x0_out(sn, mode):
    """x_prev == x_t (how diffusion.py calls it) and x0_out == NULL give the bits of the plain call."""
    i = R.make_case("ddpm_step", sn, mode=mode, obj=1, lohi=R.RANGES[0]).inp
    plain = run_ddpm_step(i)
    inplace, no_x0 = run_ddpm_step(i, inplace=True), run_ddpm_step(i, x0_out=False)
    assert torch.equal(inplace["x_prev"], plain["x_prev"]) and torch.equal(inplace["x0"], plain["x0"])
    assert torch.equal(no_x0["x_prev"], plain["x_prev"]) and bool(torch.isfinite(plain["x_prev"]).all())
    p = R.make_case("posterior_step", sn, mode=mode, lohi=R.RANGES[0]).inp
    assert torch.equal(run_posterior_step(p, inplace=True)["x_prev"], run_posterior_step(p)["x_prev"])


@pytest.mark.parametrize("sn", ["SMALL", "SMALL_C1", "LARGE"])
@pytest.mark.parametrize("lohi", R.RANGES)
def test_k2_kernels_are_the_two_branch_kernels(sn, lohi):
    """K = 2 with m_1 = 1 - (m_0 >= 1): ld_fuse_ddpm_k, ld_fuse_ddim_k and ld_branch_conditions_k give the two-branch kernels' bits."""
    from types import SimpleNamespace as NS
    i = R.make_case("fuse_ddim", sn, lohi=lohi, noz=False).inp
    k = NS(x_first=i.xo, x_rest=i.xi[None], x0_first=i.x0o, x0_rest=i.x0i[None], masks=R.masks_two(i.mask), z=i.z, k=i.k,
           lo=i.lo, hi=i.hi)
    a, b = run_fuse_ddpm(i), run_fuse_ddpm_k(k)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["x0"], b["x0"]) and bool(torch.isfinite(a["x0"]).all())
    a, b = run_fuse_ddim(i), run_fuse_ddim_k(k)
    assert torch.equal(a["x_next"], b["x_next"]) and bool(torch.isfinite(a["x_next"]).all())
    c = NS(cond=i.xo, mask=i.mask, masks=k.masks, lo_clip=R.f32(0.95))
    a, b = run_branch_conditions(c), run_branch_conditions_k(c)
    assert torch.equal(a["cond_out"], b["cond_k"][0]) and torch.equal(a["cond_in"], b["cond_k"][1])


@pytest.mark.parametrize("lo_clip", [0.5, 0.95])
@pytest.mark.parametrize("H", [28, 32])
@pytest.mark.parametrize("Cc", [1, 3])
def test_two_branch_kernels_equal_the_k_kernels_at_the_sampler_shapes(Cc, H, lo_clip):
    """The sampler calls only the ``*_k`` kernels; a single-channel mask m runs as K = 2 with masks [m, 1 - (m >= 1)].  What
    anchors "K = 2 is the reference's path" is this: on the same inputs ld_branch_conditions, ld_fuse_ddpm and ld_fuse_ddim
    (with and without a noise pointer) give the bits of ld_branch_conditions_k, ld_fuse_ddpm_k and ld_fuse_ddim_k.  B = 2 at
    the sampler's maps (28^2: HW is no power of two), masks holding 0.5 and 1.5 beside 0 and 1 (the >= 1 binarisation), and
    exact zeros planted in the states and predictions so that both arms of ``a == 0 ? c : a`` and ``a0 == 0 ? alt : a0``
    are taken on both sides (checked on the CPU with pointwise_ref's selectors)."""
    from types import SimpleNamespace as NS
    B, key = 2, 9000 + 100 * Cc + H
    s = (B, Cc, H, H)
    u = R.uni((B, 1, H, H), key, 0.0, 1.0)
    mask = torch.zeros(B, 1, H, H)
    mask[u < 0.75], mask[u < 0.50], mask[u < 0.25] = 0.5, 1.5, 1.0
    masks = R.masks_two(mask)
    assert {float(v) for v in mask.unique()} == {0.0, 0.5, 1.0, 1.5}
    for lo, hi in R.RANGES:
        xo, xi = R.values(s, key + 1, -2, 2), R.values(s, key + 2, -2, 2)
        x0o, x0i = R.values(s, key + 3, lo - 1, hi + 1), R.values(s, key + 4, lo - 1, hi + 1)
        two = NS(xo=xo, xi=xi, x0o=x0o, x0i=x0i, mask=mask, z=R.uni(s, key + 5), k=R._fuse_scalars(), lo=lo, hi=hi)
        kk = NS(x_first=xo, x_rest=xi[None], x0_first=x0o, x0_rest=x0i[None], masks=masks, z=two.z, k=two.k, lo=lo, hi=hi)
        # both arms of both selectors occur, in the two-branch and in the K-mask statement alike
        sels = [{}, {}, {}, {}]
        R.fuse_ddpm(xo, xi, x0o, x0i, mask, lo, hi, torch.float32, sels[0])
        R.fuse_ddpm_k(xo, xi[None], x0o, x0i[None], masks, lo, hi, torch.float32, sels[1])
        R.fuse_ddim(xo, xi, x0o, x0i, mask, two.z, two.k, lo, hi, torch.float32, sels[2])
        R.fuse_ddim_k(xo, xi[None], x0o, x0i[None], masks, two.z, two.k, lo, hi, torch.float32, sels[3])
        inside = (mask >= 1.0).expand(s)
        for sel, name in ((sels[0], "a==0"), (sels[1], "a0==0"), (sels[2], "a0==0"), (sels[3], "a0==0")):
            assert bool(sel[name].any()) and bool((~sel[name]).any()), (name, lo, hi)
        assert bool((sels[0]["a==0"] & inside).any()), "no exactly-zero OOD state inside the mask"
        a, b = run_fuse_ddpm(two), run_fuse_ddpm_k(kk)
        assert np.array_equal(a["x"].numpy(), b["x"].numpy()) and np.array_equal(a["x0"].numpy(), b["x0"].numpy())
        assert bool(torch.isfinite(a["x"]).all()) and bool(torch.isfinite(a["x0"]).all())
        for z in (two.z, None):
            two.z = kk.z = z
            a, b = run_fuse_ddim(two), run_fuse_ddim_k(kk)
            assert np.array_equal(a["x_next"].numpy(), b["x_next"].numpy()) and bool(torch.isfinite(a["x_next"]).all())
    c = NS(cond=R.values(s, key + 6, 0.0, 2.0), mask=mask, masks=masks, lo_clip=R.f32(lo_clip))
    a, b = run_branch_conditions(c), run_branch_conditions_k(c)
    assert np.array_equal(a["cond_out"].numpy(), b["cond_k"][0].numpy())
    assert np.array_equal(a["cond_in"].numpy(), b["cond_k"][1].numpy())
    assert bool(torch.isfinite(b["cond_k"]).all())


# ------------------------------------------------------------------------------------------------ head-of-step work
GUARD = 64                                          # floats of NaN before and after every buffer a kernel writes
RAGGED = 16 * (256 * 8 * 3 + 5)                      # bytes: the zeroing loop ends in a ragged tail
T_TABLE = [41, 33, 25, 17, 9, 1]


class Guarded:
    """``nbytes`` of NaN (never zero: the kernel must write every byte it owns) between two NaN guard bands."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = hh.nans(2 * GUARD + self.n)
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        self.nbytes = nbytes
        assert self.ptr % 16 == 0

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return g.numel() == 2 * GUARD and bool(torch.isnan(g).all())

    def zeroed(self):
        return bool((self.body().view(torch.int32) == 0).all())


class Head:
    """The buffers of one head-of-step call and what the call must leave in them."""

    def __init__(self, bytes_a, bytes_b, mode, row_floats, t0=7, idx0=2):
        self.a, self.b = Guarded(bytes_a), Guarded(bytes_b)
        self.mode, self.row_floats = mode, row_floats
        self.t = i32(5, t0, 6)                        # the counter between two neighbours that must not move
        self.idx = i32(8, idx0, 9) if mode == "table" else None
        self.table = i32(*T_TABLE) if mode == "table" else None
        self.delta = {"dec": -1, "zero": 0, "table": -1}[mode]      # (ignored in table mode)
        self.t_new = T_TABLE[idx0 + 1] if mode == "table" else t0 + self.delta
        self.idx_new = idx0 + 1
        self.rows = self.cur = None
        if row_floats:
            self.rows = R.uni((R.T, row_floats), 300 + row_floats).to(hh.DEV)
            self.cur = Guarded(4 * row_floats)

    def args(self):
        g = cabi.StepBeginArgs()
        g.zero_a, g.bytes_a, g.zero_b, g.bytes_b = self.a.ptr, self.a.nbytes, self.b.ptr, self.b.nbytes
        g.t_ptr, g.delta = self.t.data_ptr() + 4, self.delta
        g.idx_ptr = None if self.idx is None else self.idx.data_ptr() + 4
        g.t_table = P(self.table)
        g.film_rows, g.row_floats, g.film_cur = P(self.rows), self.row_floats or 0, None if self.cur is None else self.cur.ptr
        return g

    def launch(self):
        g, lib = self.args(), cabi.lib()
        if self.rows is None:
            cabi.check(lib.ld_step_begin(g.zero_a, g.bytes_a, g.zero_b, g.bytes_b, g.t_ptr, g.delta, g.idx_ptr, g.t_table, hh.st()), "step_begin")
        else:
            cabi.check(lib.ld_step_begin_film(g.zero_a, g.bytes_a, g.zero_b, g.bytes_b, g.t_ptr, g.delta, g.idx_ptr, g.t_table,
                                              g.film_rows, g.row_floats, g.film_cur, hh.st()), "step_begin_film")

    def verify(self):
        torch.cuda.synchronize()
        assert self.a.zeroed() and self.b.zeroed()
        assert self.a.guards_intact() and self.b.guards_intact()
        assert self.t.tolist() == [5, self.t_new, 6]
        if self.idx is not None:
            assert self.idx.tolist() == [8, self.idx_new, 9] and self.table.tolist() == T_TABLE
        if self.rows is not None:                    # the row of the counter AFTER the move
            assert self.cur.guards_intact()
            assert torch.equal(self.cur.body().view(torch.int32), self.rows[self.t_new].view(torch.int32))

    def state(self):
        return [t.clone() for t in (self.a.buf, self.b.buf, self.t) + (() if self.idx is None else (self.idx,))
                + (() if self.cur is None else (self.cur.buf,))]


ARENAS = [(0, 16), (16, 0), (RAGGED, 16), (16, RAGGED), (RAGGED, RAGGED)]


@pytest.mark.parametrize("row_floats", [None, 4, 1028])
@pytest.mark.parametrize("mode", ["dec", "zero", "table"])
@pytest.mark.parametrize("arenas", ARENAS, ids=lambda a: f"{a[0]}+{a[1]}")
def test_step_begin(arenas, mode, row_floats):
    h = Head(arenas[0], arenas[1], mode, row_floats)
    h.launch()
    h.verify()


def test_step_begin_without_a_counter_only_zeroes():
    a, b = Guarded(RAGGED), Guarded(16)
    cabi.check(cabi.lib().ld_step_begin(a.ptr, a.nbytes, b.ptr, b.nbytes, None, -1, None, None, hh.st()), "step_begin")
    torch.cuda.synchronize()
    assert a.zeroed() and b.zeroed() and a.guards_intact() and b.guards_intact()


def test_step_add():
    t = i32(5, 7, 6)
    for delta, want in ((-1, 6), (0, 6), (3, 9)):
        cabi.check(cabi.lib().ld_step_add(t.data_ptr() + 4, delta, hh.st()), "step_add")
        assert t.tolist() == [5, want, 6]


def test_step_begin_refuses_bad_arguments():
    """Host-side refusals: LD_EINVAL, the reason in ld_last_error, and nothing launched (every buffer keeps its NaN)."""
    lib = cabi.lib()
    a, b, cur = Guarded(32), Guarded(16), Guarded(16)
    t, idx, table = i32(7), i32(2), i32(*T_TABLE)
    rows = R.uni((R.T, 8), 310).to(hh.DEV)
    tp, ip, tt, st = t.data_ptr(), idx.data_ptr(), table.data_ptr(), hh.st()
    calls = [
        (lambda: lib.ld_step_begin(a.ptr + 4, 16, b.ptr, 16, tp, -1, None, None, st), "16-byte aligned"),
        (lambda: lib.ld_step_begin(a.ptr, 24, b.ptr, 16, tp, -1, None, None, st), "16-byte aligned"),
        (lambda: lib.ld_step_begin(a.ptr, 16, b.ptr, 16, tp, -1, ip, None, st), "idx_ptr and t_table go together"),
        (lambda: lib.ld_step_begin_film(a.ptr, 16, b.ptr, 16, tp, -1, None, None, rows.data_ptr(), 8, None, st),
         "film_rows and film_cur go together"),
        (lambda: lib.ld_step_begin_film(a.ptr, 16, b.ptr, 16, tp, -1, None, None, rows.data_ptr(), 6, cur.ptr, st), "row_floats"),
    ]
    for call, reason in calls:
        assert call() == LD_EINVAL
        assert reason in lib.ld_last_error().decode()
    g = cabi.StepBeginArgs()
    g.zero_a, g.bytes_a, g.zero_b, g.bytes_b, g.t_ptr, g.delta, g.idx_ptr, g.t_table = a.ptr + 4, 16, b.ptr, 16, tp, -1, ip, tt
    x = hh.nans(1, 1, 8, 8)
    assert lib.ld_conv_stem_begin(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 1, 8, 8, cabi.LD_BF16, C.byref(g), st) == LD_EINVAL
    assert "16-byte aligned" in lib.ld_last_error().decode()
    torch.cuda.synchronize()
    for buf in (a, b, cur):
        assert bool(torch.isnan(buf.buf).all())
    assert t.tolist() == [7] and idx.tolist() == [2]


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("arenas", [(16, 16), (RAGGED, 16), (16 * 12000, 16 * 6757)], ids=["small", "ragged", "300KB"])
@pytest.mark.parametrize("B,cin", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_conv_stem_begin(B, cin, arenas, dtype):
    """The stem convolution with the head-of-step workgroups beside it: the image is ld_conv_stem's, the side effects on
    arenas, counters and FiLM row are ld_step_begin_film's on copies, bit for bit.  The launch takes
    min(8, max(1, (units / 2048 + B) / B)) head-of-step workgroups per image for ``units`` 16-byte stores (integer
    divisions): 1 for the small arenas at either B, 4 (B = 1) and 2 (B = 3) for the ragged one, and for ~300 KB the cap
    of 8 at B = 1 and 4 at B = 3."""
    H, W, lib = 40, 33, cabi.lib()
    nbeg = min(8, max(1, ((arenas[0] + arenas[1]) // 16 // 2048 + B) // B))
    assert nbeg == {(16, 16): {1: 1, 3: 1}, (RAGGED, 16): {1: 4, 3: 2}, (16 * 12000, 16 * 6757): {1: 8, 3: 4}}[arenas][B]
    x, w, b = R.uni((B, cin, H, W), 320).to(hh.DEV), R.uni((32, cin, 7, 7), 321, -0.3, 0.3).to(hh.DEV), R.uni((32,), 322).to(hh.DEV)
    wp = torch.zeros(int(lib.ld_stem_packed_bytes()), dtype=torch.uint8, device=hh.DEV)
    cabi.check(lib.ld_pack_stem_weight(w.data_ptr(), wp.data_ptr(), cin, hh.st()), "pack_stem")
    code = cabi.dtype_code(dtype)
    want = hh.nans(B, H, W, 32, dtype=hh.TDT[dtype])
    cabi.check(lib.ld_conv_stem(x.data_ptr(), wp.data_ptr(), b.data_ptr(), want.data_ptr(), B, cin, H, W, code, hh.st()), "conv_stem")
    assert bool(torch.isfinite(want.float()).all())
    for mode, row_floats in (("dec", 1028), ("table", 4), ("zero", None)):
        alone, fused = Head(arenas[0], arenas[1], mode, row_floats), Head(arenas[0], arenas[1], mode, row_floats)
        alone.launch()
        alone.verify()
        out = hh.nans(B, H, W, 32, dtype=hh.TDT[dtype])
        g = fused.args()
        cabi.check(lib.ld_conv_stem_begin(x.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), B, cin, H, W, code,
                                          C.byref(g), hh.st()), "conv_stem_begin")
        fused.verify()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))
        for u, v in zip(alone.state(), fused.state()):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the fused final step
def _final_step_pair(x, w, b, xt, sched, mask, t, obj, lo, hi, B, H, W, cin, cout, dtype):
    """(fused ld_final_step_at, the separate launches ld_final_conv, ld_mask_out, ld_randn_at, ld_ddpm_step) -> two triples."""
    lib, code, n, seed, base, tmul = cabi.lib(), cabi.dtype_code(dtype), xt.numel(), 10, 100, -1
    tdev = i32(t)
    mo1, x1, x01 = torch.full_like(xt, hh.NAN), xt.clone(), torch.full_like(xt, hh.NAN)
    cabi.check(lib.ld_final_step_at(x.data_ptr(), w.data_ptr(), b.data_ptr(), mo1.data_ptr(), x1.data_ptr(), x01.data_ptr(),
                                    sched.data_ptr(), tdev.data_ptr(), lo, hi, obj, seed, base, tmul, 0, P(mask), B, H, W, cin, cout,
                                    code, hh.st()), "final_step_at")
    mo2, x2, x02, z = torch.full_like(xt, hh.NAN), torch.full_like(xt, hh.NAN), torch.full_like(xt, hh.NAN), torch.full_like(xt, hh.NAN)
    cabi.check(lib.ld_final_conv(x.data_ptr(), w.data_ptr(), b.data_ptr(), mo2.data_ptr(), B, H, W, cin, cout, code, hh.st()), "final_conv")
    if mask is not None:
        cabi.check(lib.ld_mask_out(mo2.data_ptr(), mask.data_ptr(), lo, B, cout, H * W, hh.st()), "mask_out")
    cabi.check(lib.ld_randn_at(z.data_ptr(), n, 0, seed, base, tmul, tdev.data_ptr(), hh.st()), "randn_at")
    cabi.check(lib.ld_ddpm_step(xt.data_ptr(), mo2.data_ptr(), z.data_ptr(), x2.data_ptr(), x02.data_ptr(), sched.data_ptr(),
                                tdev.data_ptr(), lo, hi, obj, n, hh.st()), "ddpm_step")
    return (mo1, x1, x01), (mo2, x2, x02)


def _final_inputs(B, H, W, cin, cout, dtype):
    x = hh.nhwc(R.uni((B, cin, H, W), 330), dtype)
    w, b = R.uni((cout, cin), 331, -0.3, 0.3).to(hh.DEV), R.uni((cout,), 332).to(hh.DEV)
    sched = R.uni((20, 8), 333, 0.1, 0.9).to(hh.DEV)
    return x, w, b, R.uni((B, cout, H, W), 334).to(hh.DEV), sched, R.mask2(B, H, W, 335).to(hh.DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", [1, 2, 4])
@pytest.mark.parametrize("cin", [8, 24, 32, 40])
def test_final_step_at_is_the_separate_launches(cin, cout, dtype):
    """With and without keep_mask, three objectives, t = 0 (no draw) and t = 7: model_out, x_t and x0 bit for bit."""
    B, H, W = 2, 9, 11
    x, w, b, xt, sched, mask = _final_inputs(B, H, W, cin, cout, dtype)
    for keep in (None, mask):
        for obj in range(3):
            for t in (0, 7):
                lo, hi = R.RANGES[obj % 2]
                fused, sep = _final_step_pair(x, w, b, xt, sched, keep, t, obj, lo, hi, B, H, W, cin, cout, dtype)
                for u, v in zip(fused, sep):
                    assert torch.equal(u, v) and bool(torch.isfinite(u).all()), (keep is not None, obj, t)
                if keep is not None:                 # the mask reaches the model output
                    assert bool((fused[0] == lo).any()) and bool((fused[0] != lo).any())


def test_final_step_at_past_the_grid_cap():
    """1025 x 1025 pixels: more than 4096 * 256, so the pixel loop of both kernels makes a second trip."""
    B, H, W, cin, cout, dtype = 1, 1025, 1025, 8, 2, "bf16"
    assert B * H * W > R.CAP
    x, w, b, xt, sched, mask = _final_inputs(B, H, W, cin, cout, dtype)
    fused, sep = _final_step_pair(x, w, b, xt, sched, mask, 7, 1, 0.0, 2.0, B, H, W, cin, cout, dtype)
    for u, v in zip(fused, sep):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())
