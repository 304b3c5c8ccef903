"""tests/pointwise_ref.py proved on the CPU: the references against oracle/diffusion_ref.py, the K = 2 reduction of the
K-mask rules, the preconditions of the input builders, the measured error ``d`` of the fp32 restatement that the GPU
tolerance of tests/test_hip_pointwise.py is taken from, and the mutation check: every subtly wrong kernel below, applied
to the fp32 restatement, fails the GPU tests' own comparison (pointwise_ref.passes) on the same inputs and bound."""
import copy
from types import SimpleNamespace

import pytest
import torch

from oracle import diffusion_ref as O
import pointwise_ref as R

F32, F64 = torch.float32, torch.float64
CASES = R.case_list()


def _n(case):
    B, C, H, W = case.shape
    return B * C * H * W


# ------------------------------------------------------------------------------------------------ builders, d, generic mutants
def _unwritten(case, first, count):
    """The fp32 restatement with elements [first, first + count) of the kernel's index space never stored (NaN fill)."""
    n, out = _n(case), {}
    for name, t in case.ref32.items():
        t = t.clone()
        if t.numel() % n == 0:
            t.reshape(-1, n)[:, first:first + count] = float("nan")
        out[name] = t
    return out


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_case(c):
    kernel, sn, v = c
    case = R.make_case(kernel, sn, **v)
    n = _n(case)
    # every arm of every == 0 selection is taken by >= 1 % of the elements, and both precisions take the same arm
    assert case.sel32.keys() == case.sel64.keys()
    for name, s in case.sel32.items():
        assert torch.equal(s, case.sel64[name]), (name, int((s != case.sel64[name]).sum()))
        frac = float(s.float().mean())
        assert 0.01 <= frac <= 0.99, (name, frac)
    # the planted edges
    inp = vars(case.inp)
    for name in ("x", "xo", "xi", "x_first", "x_rest", "mo", "x0o", "x0i", "x0_first", "x0_rest"):
        if name in inp and kernel not in ("q_sample_t", "p_losses"):
            z = inp[name] == 0.0
            assert bool((z & ~torch.signbit(inp[name])).any()) and bool((z & torch.signbit(inp[name])).any()), name
    if "lohi" in v:
        for name in ("mo", "x0o", "x0i", "x0_first", "x0_rest"):
            if name in inp:
                assert float((inp[name] < v["lohi"][0]).float().mean()) >= 0.01 and float((inp[name] > v["lohi"][1]).float().mean()) >= 0.01
    if "mask" in inp:
        assert sorted(torch.unique(inp["mask"]).tolist()) == [0.0, R.f32(0.7), 1.0, 1.5]
    if "masks" in inp and kernel != "recompose":
        owners = (inp["masks"] >= 1.0).sum(1)
        for count in (0, 1, 2):                          # pixels owned by no branch, by one and by two: >= 1 % each
            assert float((owners == count).float().mean()) >= 0.01, (count, float((owners == count).float().mean()))
    # the measured error of the fp32 restatement: what the GPU tolerance is taken from
    for name, d in case.d.items():
        if name in case.each:
            for b, bnd in enumerate(R.bound_each(case.ref64[name], case.d_each[name]).tolist()):
                print(f"d {R.case_id(c)} {name}[{b}]: {float(case.d_each[name][b]):.3e} (bound {bnd:.3e}, |ref| {float(case.ref64[name][b].abs()):.6e})")
            continue
        print(f"d {R.case_id(c)} {name}: {d:.3e} (bound {R.bound(case.ref64[name], d):.3e}, max |ref| {float(case.ref64[name].abs().max()):.3e})")
    assert R.passes(case, case.ref32)
    # mutants every kernel shares: the last n % 256 elements, and everything past the first trip of the capped grid
    if any(t.numel() % n == 0 for t in case.ref32.values()):
        assert n % 256 != 0
        assert not R.passes(case, _unwritten(case, n - n % 256, n % 256))
        assert not R.passes(case, _unwritten(case, n - 1, 1))
        if n > R.CAP:
            assert not R.passes(case, _unwritten(case, R.CAP, n - R.CAP))
    # an output held to the bound sample by sample: a wrong value in any one sample fails, the smallest included (the
    # losses of t = T - 1 and t = 0 lie seven decades apart, and one bound for the vector would be several times the smallest)
    for name in case.each:
        ref32 = case.ref32[name]
        per = n // ref32.numel()
        assert float(case.ref64[name].abs().min()) > 0.0
        for b in range(ref32.numel()):
            for wrong in (0.0, float(ref32[b]) * (1.0 + 1e-5)):        # (1e-5 is ~84 ulp: 4 d_b is at most a few)
                got = ref32.clone()
                got[b] = wrong
                assert not R.passes(case, {**case.ref32, name: got}), (b, wrong)
            # the last per % 256 elements of sample b left out of its sum (all three inputs zero there: a zero difference)
            cut = {k: getattr(case.inp, k).clone() for k in ("mo", "x0", "z")}
            for t in cut.values():
                t[b].reshape(-1)[per - per % 256:] = 0.0
            assert per % 256 != 0 and not R.passes(case, _ref32(case, **cut)), b


# ------------------------------------------------------------------------------------------------ mutation check
def _ref32(case, **changed):
    inp = copy.copy(case.inp)
    for k, val in changed.items():
        setattr(inp, k, val)
    return case.ref(inp, F32)


def _flip(mask):
    return torch.where(mask >= 1.0, 0.0, 1.0)


def mutant(case, name):
    i, (B, C, H, W) = case.inp, case.shape
    if name == "swap_m":                                   # m and 1 - m swapped
        return _ref32(case, mask=_flip(i.mask))
    if name == "last_branch":                              # the last non-zero of the further branches instead of the first
        return _ref32(case, x_rest=i.x_rest.flip(0), x0_rest=i.x0_rest.flip(0),
                      masks=torch.cat([i.masks[:, :1], i.masks[:, 1:].flip(1)], 1))
    if name == "no_branch_clamp":                          # fuse_ddpm without the per-branch clamp
        out = dict(case.ref32)
        m = (i.mask >= 1.0).float()
        out["x0"] = (i.x0i * (1.0 - m) + i.x0o).clamp(i.lo, i.hi)
        return out
    if name == "noise_at_t0":                              # the draw added at t == 0
        return _ref32(case, t=None, sched=i.sched[0:1])
    if name == "row_off_by_one":
        return _ref32(case, idx=i.idx + 1) if hasattr(i, "idx") else _ref32(case, t=i.t + 1)
    if name == "batch_index":                              # b = i / HW without / C: channel plane bc reads mask plane bc (mod B)
        bc = torch.arange(B * C) % B
        return _ref32(case, mask=i.mask[bc, 0].reshape(B, C, H, W))
    raise KeyError(name)


MUTANTS = [
    ("swap_m", "branch_conditions", "SMALL", dict(lo_clip=R.f32(0.95))),
    ("swap_m", "mask_out", "SMALL", dict(lohi=R.RANGES[0])),
    ("swap_m", "fuse_ddpm", "SMALL", dict(lohi=R.RANGES[0])),
    ("swap_m", "fuse_ddpm", "LARGE", dict(lohi=R.RANGES[1])),
    ("swap_m", "fuse_ddim", "SMALL", dict(lohi=R.RANGES[0], noz=False)),
    ("last_branch", "fuse_ddpm_k", "SMALL", dict(K=3, lohi=R.RANGES[0])),
    ("last_branch", "fuse_ddpm_k", "SMALL", dict(K=5, lohi=R.RANGES[1])),
    ("last_branch", "fuse_ddim_k", "SMALL", dict(K=3, lohi=R.RANGES[0], noz=False)),
    ("last_branch", "fuse_ddim_k", "LARGE", dict(K=3, lohi=R.RANGES[1], noz=False)),
    ("no_branch_clamp", "fuse_ddpm", "SMALL", dict(lohi=R.RANGES[0])),
    ("no_branch_clamp", "fuse_ddpm", "SMALL_C1", dict(lohi=R.RANGES[1])),
    ("noise_at_t0", "ddpm_step", "SMALL", dict(mode="t0", obj=0, lohi=R.RANGES[0])),
    ("noise_at_t0", "ddpm_step", "LARGE", dict(mode="t0", obj=0, lohi=R.RANGES[0])),
    ("noise_at_t0", "posterior_step", "SMALL", dict(mode="t0", lohi=R.RANGES[0])),
    ("row_off_by_one", "ddpm_step", "SMALL", dict(mode="t1", obj=1, lohi=R.RANGES[0])),
    ("row_off_by_one", "ddpm_step", "SMALL", dict(mode="t1", obj=0, lohi=R.RANGES[1])),
    ("row_off_by_one", "posterior_step", "SMALL", dict(mode="t1", lohi=R.RANGES[0])),
    ("row_off_by_one", "ddim_step", "SMALL", dict(variant="plain", obj=2, lohi=R.RANGES[0])),
    ("row_off_by_one", "ddim_step", "LARGE", dict(variant="plain", obj=0, lohi=R.RANGES[1])),
    ("batch_index", "branch_conditions", "SMALL", dict(lo_clip=R.f32(0.95))),
    ("batch_index", "mask_out", "SMALL", dict(lohi=R.RANGES[1])),
    ("batch_index", "fuse_ddpm", "SMALL", dict(lohi=R.RANGES[0])),
    ("batch_index", "fuse_ddim", "SMALL", dict(lohi=R.RANGES[0], noz=False)),
    ("batch_index", "fuse_ddim", "LARGE", dict(lohi=R.RANGES[0], noz=False)),
]


@pytest.mark.parametrize("m", MUTANTS, ids=lambda m: m[0] + "-" + R.case_id(m[1:]))
def test_mutant_fails_the_gpu_comparison(m):
    name, kernel, sn, v = m
    assert (kernel, sn, v) in CASES                        # a case the GPU test runs, with its bound
    case = R.make_case(kernel, sn, **v)
    got = mutant(case, name)
    res = R.errors(case, got)
    assert not all(ok for ok, _, _ in res.values()), res
    assert R.passes(case, case.ref32)


# ------------------------------------------------------------------------------------------------ K = 2 reduction
@pytest.mark.parametrize("sn", ["SMALL", "SMALL_C1", "LARGE"])
@pytest.mark.parametrize("lohi", R.RANGES)
def test_k2_is_the_two_branch_rule(sn, lohi):
    """K = 2 with m_1 = 1 - (m_0 >= 1): the K-mask references give the two-branch ones bit for bit in fp32."""
    lo, hi = lohi
    i = R.make_case("fuse_ddim", sn, lohi=lohi, noz=False).inp
    m2 = R.masks_two(i.mask)
    a = R.fuse_ddpm(i.xo, i.xi, i.x0o, i.x0i, i.mask, lo, hi, F32)
    b = R.fuse_ddpm_k(i.xo, i.xi[None], i.x0o, i.x0i[None], m2, lo, hi, F32)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["x0"], b["x0"])
    a = R.fuse_ddim(i.xo, i.xi, i.x0o, i.x0i, i.mask, i.z, i.k, lo, hi, F32)
    b = R.fuse_ddim_k(i.xo, i.xi[None], i.x0o, i.x0i[None], m2, i.z, i.k, lo, hi, F32)
    assert torch.equal(a["x_next"], b["x_next"])
    a = R.branch_conditions(i.xo, i.mask, R.f32(0.95), F32)
    b = R.branch_conditions_k(i.xo, m2, R.f32(0.95), F32)
    assert torch.equal(a["cond_out"], b["cond_k"][0]) and torch.equal(a["cond_in"], b["cond_k"][1])


# ------------------------------------------------------------------------------------------------ against the oracle
class Stub:
    """A denoiser that returns prepared outputs in call order and keeps the states it was given."""

    def __init__(self, outs):
        self.outs, self.seen = list(outs), []

    def __call__(self, x, cond, t):
        self.seen.append((x, cond))
        return self.outs[len(self.seen) - 1]


class Draws:
    def __init__(self, zs):
        self.zs, self.k = list(zs), 0

    def __call__(self, shape):
        self.k += 1
        return self.zs[self.k - 1]


def _sampler(f=None, objective="pred_x0", shape=R.SHAPES["SMALL"], **kw):
    rs = O.RefSampler(f, O.SamplerOptions(timesteps=R.T, objective=objective, **kw), shape[1], shape[2])
    for name, t in R.sched_table(objective)[1].items():                    # the package's buffers: bit-equal to the oracle's
        assert torch.equal(rs.buf[name], t), name
    return rs


def _close(a, b):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12, float((a - b).abs().max())


SMALL_SHAPES = ["SMALL", "SMALL_C1"]


@pytest.mark.parametrize("sn", SMALL_SHAPES)
def test_branch_conditions_against_the_oracle(sn):
    """The oracle rounds its conditions to fp32 (.float()), so the fp32 forms are compared, bit for bit, and the fp64 form
    of the hard-masked branch (a product with 0 / 1) to 1e-12."""
    i = R.make_case("branch_conditions", sn, lo_clip=R.f32(0.95)).inp
    rs = _sampler(shape=R.SHAPES[sn])
    _, co, ci = rs.branch_conditions(i.cond, i.mask)
    mine = R.branch_conditions(i.cond, i.mask, R.f32(0.95), F32)
    assert torch.equal(mine["cond_out"], co) and torch.equal(mine["cond_in"], ci)
    _close(R.branch_conditions(i.cond, i.mask, R.f32(0.95), F64)["cond_out"], co.double())
    rs = _sampler(shape=R.SHAPES[sn], data="mnist")                          # lo_clip 0.5
    _, co, ci = rs.branch_conditions(i.cond, i.mask)
    mine = R.branch_conditions(i.cond, i.mask, 0.5, F32)
    assert torch.equal(mine["cond_out"], co) and torch.equal(mine["cond_in"], ci)
    for K in (2, 3, 5):
        ik = R.make_case("branch_conditions_k", sn, K=K, lo_clip=R.f32(0.95)).inp
        _, conds = _sampler(shape=R.SHAPES[sn]).kmask_conditions(ik.cond, ik.masks)
        assert torch.equal(R.branch_conditions_k(ik.cond, ik.masks, R.f32(0.95), F32)["cond_k"], torch.stack(conds))


@pytest.mark.parametrize("sn", SMALL_SHAPES)
@pytest.mark.parametrize("lohi", R.RANGES)
@pytest.mark.parametrize("K", [2, 3, 5])
def test_kmask_fuse_against_the_oracle(sn, lohi, K):
    i = R.make_case("fuse_ddpm_k", sn, K=K, lohi=lohi).inp
    rs = _sampler(shape=R.SHAPES[sn])
    xs = [i.x_first.double()] + [t.double() for t in i.x_rest]
    x0s = [i.x0_first.double().clamp(*lohi)] + [t.double().clamp(*lohi) for t in i.x0_rest]      # kmask_predict clamps every branch
    x, x0 = rs.kmask_fuse(xs, x0s, (i.masks >= 1.0).float(), lohi)
    mine = R.fuse_ddpm_k(i.x_first, i.x_rest, i.x0_first, i.x0_rest, i.masks, lohi[0], lohi[1], F64)
    _close(mine["x"], x)
    _close(mine["x0"], x0)


@pytest.mark.parametrize("sn", SMALL_SHAPES)
@pytest.mark.parametrize("lohi", R.RANGES)
def test_fuse_step_against_the_oracle(sn, lohi):
    """_fuse_step at t = 0 (no draw) with a stub denoiser: its recomposition lines are fuse_ddpm, its return value is
    posterior_step of the fused pair, and mask_x is mask_out."""
    i = R.make_case("fuse_ddpm", sn, lohi=lohi).inp
    for mask_x in (False, True):
        stub = Stub([i.x0i.double(), i.x0o.double()])                        # predict_branches evaluates the IND branch first
        rs = _sampler(stub, shape=R.SHAPES[sn])
        x0o = R.mask_out(i.x0o, i.mask, lohi[0], F64)["model_out"] if mask_x else i.x0o.double()
        mine = R.fuse_ddpm(i.xo.double(), i.xi.double(), x0o, i.x0i.double(), i.mask, lohi[0], lohi[1], F64)
        for t in (0, 3):
            stub.seen = []
            z = R.uni(i.xo.shape, 12, -2, 2)
            sigma = (0.5 * rs.buf["posterior_log_variance_clipped"][t]).exp()
            ret, x0, (xo, xi) = rs._fuse_step([i.xo.double(), i.xi.double()], i.xo, i.mask, t, lohi, mask_x, Draws([z.double()]), sigma)
            _close(mine["x0"], x0)
            _close(mine["x"], torch.where(xo == 0.0, xi, xo))
            _close(R.posterior_step(mine["x"], mine["x0"], z, R.sched_table()[0], t, F64)["x_prev"], ret)
        _close(R.posterior_step(i.xo, i.x0o, None, R.sched_table()[0], 7, F64)["x_prev"], rs.posterior_mean(i.x0o.double(), i.xo.double(), 7))


def _ddim_run(sn, lohi, K, eta=0.5):
    """Three DDIM pairs (49 -> 32 -> 15 -> -1) with start_timestep = 1: the first is a branch step (ddim_step per branch),
    the second fuses, and the third hands the fused state to the stub denoiser, where it is read."""
    B, C, H, W = R.SHAPES[sn]
    s = (B, C, H, W)
    nb = 2 if K is None else K
    p1 = [R.values(s, 200 + k, lohi[0] - 1, lohi[1] + 1).double() for k in range(nb)]
    p2 = [R.values(s, 210 + k, lohi[0] - 1, lohi[1] + 1).double() for k in range(nb)]
    xT, z1, z2 = [R.uni(s, 220 + k, -2, 2).double() for k in range(3)]
    cond = R.values(s, 230, 0, 2)
    if K is None:       # predict_branches: IND first, then OOD
        stub, mask = Stub([p1[1], p1[0], p2[1], p2[0], torch.zeros(s, dtype=F64)]), R.mask2(B, H, W, 231)
    else:               # kmask_predict: branches 1.., then branch 0
        stub, mask = Stub(p1[1:] + p1[:1] + p2[1:] + p2[:1] + [torch.zeros(s, dtype=F64)]), R.masks_k(B, K, H, W, 231)
    rs = _sampler(stub, shape=R.SHAPES[sn], sampling_timesteps=3, ddim_sampling_eta=eta, branch_out=True,
                  start_intermediate=True, start_timestep=1)
    if K is None:
        rs.ddim_sample(cond, mask, lohi, s, Draws([xT, z1, z2]), True, True, False)
    else:
        rs.ddim_sample_kmask(cond, mask, lohi, s, Draws([xT, z1, z2]), True, False)
    assert len(stub.seen) == 2 * nb + 1
    buf = R.sched_table()[1]
    k1, k2 = R.ddim_scalars(buf, 49, 32, eta), R.ddim_scalars(buf, 32, 15, eta)
    xs = [R.ddim_step(xT, p1[k], z1, k1, lohi[0], lohi[1], 0, F64)["x_next"] for k in range(nb)]
    return SimpleNamespace(xs=xs, p2=p2, z2=z2, mask=mask, k=[k2[0], k2[1], k2[4], k2[5], k2[6]], fused=stub.seen[-1][0],
                           seen=stub.seen)


@pytest.mark.parametrize("sn", SMALL_SHAPES)
@pytest.mark.parametrize("lohi", R.RANGES)
def test_ddim_fusion_against_the_oracle(sn, lohi):
    r = _ddim_run(sn, lohi, None)
    _close(r.xs[1], r.seen[2][0])                        # the branch step is ddim_step (pred_x0) per branch
    _close(r.xs[0], r.seen[3][0])
    mine = R.fuse_ddim(r.xs[0], r.xs[1], r.p2[0], r.p2[1], r.mask, r.z2, r.k, lohi[0], lohi[1], F64)
    _close(mine["x_next"], r.fused)


@pytest.mark.parametrize("sn", SMALL_SHAPES)
@pytest.mark.parametrize("lohi", R.RANGES)
@pytest.mark.parametrize("K", [2, 3, 5])
def test_ddim_kmask_fusion_against_the_oracle(sn, lohi, K):
    r = _ddim_run(sn, lohi, K)
    mine = R.fuse_ddim_k(r.xs[0], torch.stack(r.xs[1:]), r.p2[0], torch.stack(r.p2[1:]), r.mask, r.z2, r.k, lohi[0], lohi[1], F64)
    _close(mine["x_next"], r.fused)


@pytest.mark.parametrize("objective", R.OBJ_NAMES)
def test_q_sample_and_p_losses_against_the_oracle(objective):
    obj = R.OBJ_NAMES.index(objective)
    i = R.make_case("p_losses", "PER189", obj=obj, lohi=R.RANGES[obj % 2]).inp
    rs = _sampler(lambda x, cond, t: i.mo.double(), objective=objective)
    t = i.t.long()
    _close(R.q_sample_t(i.x0, i.z, t, i.sab, i.s1mab, F64)["x"], rs.q_sample(i.x0.double(), t, i.z.double()))
    _, loss = rs.p_losses(i.x0.double(), None, t, i.z.double())
    _close(R.p_losses(i.mo, i.x0, i.z, t, i.sab, i.s1mab, i.lw, obj, F64)["loss"], loss)
    q = R.make_case("q_sample", "SMALL", lohi=R.RANGES[0]).inp
    tt = torch.full((q.x0.shape[0],), R.ROW_T)
    _close(R.q_sample(q.x0, q.z, q.sab, q.s1mab, F64)["x"], rs.q_sample(q.x0.double(), tt, q.z.double()))


@pytest.mark.parametrize("objective", R.OBJ_NAMES)
def test_ddpm_and_ddim_steps_against_the_oracle(objective):
    """x0 of the three objectives (x0_from_eps / x0_from_v), eps_from_x0, the posterior mean and the DDIM update."""
    obj = R.OBJ_NAMES.index(objective)
    lohi = R.RANGES[0]
    rs = _sampler(objective=objective)
    i = R.make_case("ddpm_step", "SMALL", mode="t1", obj=obj, lohi=lohi).inp
    table, buf = R.sched_table(objective)
    x, mo = i.x.double(), i.mo.double()

    def oracle_x0(t):
        x0 = mo if obj == 0 else (rs.x0_from_eps(x, t, mo) if obj == 1 else rs.x0_from_v(x, t, mo))
        return x0.clamp(*lohi)

    for t in (0, 1, R.T - 1):
        x0 = oracle_x0(t)
        want = rs.posterior_mean(x0, x, t)
        if t > 0:
            want = want + (0.5 * rs.buf["posterior_log_variance_clipped"][t]).exp() * i.z.double()
        mine = R.ddpm_step(i.x, i.mo, i.z, table, t, lohi[0], lohi[1], obj, F64)
        _close(mine["x0"], x0)
        _close(mine["x_prev"], want)
    t, tn, eta = 32, 15, 0.5
    k = R.ddim_scalars(buf, t, tn, eta)
    x0 = oracle_x0(t)
    eps = rs.eps_from_x0(x, t, x0)
    want = x0 * k[4] + k[5] * eps + k[6] * i.z.double()
    _close(R.ddim_step(i.x, i.mo, i.z, k, lohi[0], lohi[1], obj, F64)["x_next"], want)
