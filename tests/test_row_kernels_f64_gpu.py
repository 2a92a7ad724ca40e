"""Float64 parity of the small row kernels (catops.hip, headops.hip, optim.hip) at the shapes where they can go wrong.

Every comparison is one HIP kernel, called through dv3hip.ops, against a plain float64 PyTorch expression of the same
operation on the CPU; gradients are torch.autograd's on that expression.  Inputs are seeded fp32 tensors cast to
float64 for the reference, so both sides see the same numbers.  The `dt` argument of the reference functions exists
so that the same expression can be evaluated in fp32 on the CPU: that is how the fp32 oracle's own error against
float64 was measured for the bars below (never from a kernel).

What each group pins (the gaps tests/test_kernels_gpu.py leaves open):
  * entry points with no kernel-level test: actor_loss (three objectives, `mix`, the max(., 1) of the EMA scale),
    dot_accumulate (w / clip_min / scale), scale_neg, axpby, concat_flat;
  * adam_step with weight_decay and grad_scale (decay -> clip on the SCALED norm -> step), and a step count that starts
    at 999 as a checkpoint load leaves it;
  * the second trip of every capped grid-stride loop (the `wrap` cases: sizes just above grid cap x work per block);
  * all five group widths of DV3_G_DISPATCH (D = 1, 2, 3, 4 | 8 | 16 | 17, 32 | 33, 64), last blocks partly filled
    (R = 77), kl_* with S below / not a multiple of the 64/G groups a wave packs;
  * saturated softmax / sigmoid, softplus on both sides of its z > 20 switch, the actor's absmax clip on both sides
    of 1 at min_std and max_std, continue-logits of +-50 in the discount product.

Bars: 1e-4 * max(1, max|ref|) (TOL of tests/test_kernels_gpu.py); KL gradients and Adam parameters keep the 1e-5 of
their existing tests, the sums of squares the 2e-6 of the sum of test_gradient_norm_is_summed_in_a_fixed_order.  Where
a tensor's values are far below 1 (gradients of a mean, Adam's moments) the comparison is against the tensor's own
maximum; where one row dwarfs the others (the DiscDist mode at symexp(20)) symlog of the output and a bar per row are
checked as well.  Draws: the kernel's class must equal the float64 argmax of p_hat / q on every row except rows whose
float64 top-two scores are within 1e-5 relative (asserted to be at most 1e-3 of the rows; the only place anything is
excluded).  No bar here is widened: on every case below the fp32 CPU oracle's own error against float64
stays under half the bar (measured with the same reference functions at dt=float32).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dv3_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4        # outputs and gradients (BASELINE.json north star)
TOL_KL_GRAD = 1e-5  # tests/test_kernels_gpu.py::test_kl_fwd_bwd
TOL_ADAM = 1e-5   # tests/test_kernels_gpu.py::test_adam_clip_matches_oracle
TOL_SUMSQ = 2e-6  # tests/test_kernels_gpu.py::test_gradient_norm_is_summed_in_a_fixed_order, relative to the sum
F32, F64 = torch.float32, torch.float64
U = 0.01          # unimix
TIE_REL, TIE_CAP = 1e-5, 1e-3
ALL_D = [1, 2, 3, 4, 8, 16, 17, 32, 33, 64]
KINDS = ["randn", "wide", "edge"]


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def dev(x):
    return x.cuda()


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def check(got, ref, tol=TOL, what="", floor=1.0):
    """max |got - ref| <= tol * max(floor, max |ref|); floor = 0 where the values are far below 1 (a mean's gradients)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    bar = tol * max(floor, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"{what}: max err {err:.3e} bar {bar:.3e}")
    assert err <= bar, f"{what}: max err {err:.3e} > bar {bar:.3e}"


def check_rows(got, ref, scale, tol=TOL, what=""):
    """As check(), row by row: row r is held to tol * max(1, scale[r]), so that a row of large values does not set the
    bar for the others."""
    got = got.detach().cpu().double().reshape(ref.shape[0], -1)
    ref = ref.detach().cpu().double().reshape(ref.shape[0], -1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().amax(-1)
    bar = tol * scale.detach().cpu().double().clamp_min(1.0)
    worst = int((err / bar).argmax())
    print(f"{what}: worst row {worst} max err {err[worst].item():.3e} bar {bar[worst].item():.3e}")
    assert (err <= bar).all(), f"{what}: row {worst} max err {err[worst].item():.3e} > bar {bar[worst].item():.3e}"


# ====================================================================================== categorical (catops.hip)
def cat_logits(R, D, kind, g):
    """randn: 2 randn.  wide: 30 randn (saturated softmax).  edge: row 0 all equal, row 1 a single +80, row 2 two
    equal maxima (D >= 2; the mode must take the lower index)."""
    if kind == "wide":
        return 30 * torch.randn(R, D, generator=g)
    l = 2 * torch.randn(R, D, generator=g)
    if kind == "edge":
        l[0] = 0.7
        l[1, D // 2] = 80.0
        if D >= 2:
            l[2, 1 if D > 2 else 0] = l[2, D - 1] = 9.0
    return l


def ref_probs(logit, dt=F64):
    """p_hat of tools.OneHotDist: (1 - u) softmax + u / D (as the distribution holds it after renormalising)."""
    return F.softmax(O.unimix_logits(logit.to(dt), U), -1)


def ref_draw(logit, q, dt=F64):
    """-> (class of the draw [R], near-tie mask [R]): argmax p_hat / q and whether its top-two are within TIE_REL."""
    s = ref_probs(logit, dt) / q.to(dt)
    idx = O.onehot_sample(logit.to(dt), q.to(dt), U).detach().argmax(-1)
    assert torch.equal(idx, s.argmax(-1))
    if logit.shape[-1] < 2:
        return idx, torch.zeros(logit.shape[0], dtype=torch.bool)
    top = s.topk(2, -1).values
    return idx, (top[:, 0] - top[:, 1]) < TIE_REL * top[:, 0]


def ref_mode(logit, dt=F64):
    return O.onehot_mode(logit.to(dt), U).detach().argmax(-1)


def ref_st_bwd(logit, gs, mode, dt=F64):
    l = logit.to(dt).requires_grad_(True)
    out = O.onehot_mode(l, U) if mode else O.onehot_sample(l, torch.ones_like(l), U)
    out.backward(gs.to(dt))
    return l.grad


def ref_ent_logp(logit, x, dent=None, dlogp=None, dt=F64):
    """-> (entropy [R], logp [R], dlogit [R,D] for the upstreams given)."""
    l = logit.to(dt).requires_grad_(True)
    ent = O.onehot_entropy(l[:, None, :], U)
    lp = O.onehot_logprob(l, x.to(dt), U)
    grad = torch.zeros_like(l)
    tot = 0.0
    if dent is not None:
        tot = tot + (ent * dent.to(dt)).sum()
    if dlogp is not None:
        tot = tot + (lp * dlogp.to(dt)).sum()
    if dent is not None or dlogp is not None:
        (grad,) = torch.autograd.grad(tot, l)
    return ent.detach(), lp.detach(), grad


def run_sample_checks(ops, logit, g, what):
    R, D = logit.shape
    q = torch.empty(R, D).exponential_(generator=g)
    idx_ref, near = ref_draw(logit, q)
    assert near.sum().item() <= TIE_CAP * R, f"{what}: {int(near.sum())} near-tie rows of {R}"
    ld = dev(logit)
    out = dev(torch.full((R, D), 7.0))
    idx = dev(torch.full((R,), -1, dtype=torch.int32))
    ops.onehot_sample(ld, out, noise=dev(q), idx=idx, unimix=U)
    oc, ic = out.cpu(), idx.cpu().long()
    assert torch.equal(oc, F.one_hot(ic, D).float()), f"{what}: output is not the one-hot of idx"
    bad = (ic != idx_ref) & ~near
    assert not bad.any(), f"{what}: {int(bad.sum())} draws differ from the float64 argmax (first row {int(bad.nonzero()[0])})"
    out.fill_(7.0)
    idx.fill_(-1)
    ops.onehot_sample(ld, out, idx=idx, unimix=U, mode=True)
    mref = ref_mode(logit)
    assert torch.equal(idx.cpu().long(), mref), f"{what}: mode differs from the float64 argmax"
    assert torch.equal(out.cpu(), F.one_hot(mref, D).float())
    return ld


def run_st_bwd_checks(ops, logit, ld, g, what):
    R, D = logit.shape
    gs = torch.randn(R, D, generator=g)
    base = torch.randn(R, D, generator=g)
    for mode in (False, True):
        ref = ref_st_bwd(logit, gs, mode)
        for acc in (False, True):
            dl = dev(base.clone())
            ops.onehot_st_bwd(ld, dev(gs), dl, unimix=U, mode=mode, accumulate=acc)
            check(dl, ref + base.double() if acc else ref, what=f"{what} st_bwd mode={mode} acc={acc}")


def run_ent_logp_checks(ops, logit, ld, g, what, combos):
    R, D = logit.shape
    x = F.one_hot(torch.randint(0, D, (R,), generator=g), D).float()
    de, dp = torch.randn(R, generator=g), torch.randn(R, generator=g)
    base = torch.randn(R, D, generator=g)
    ent_ref, lp_ref, _ = ref_ent_logp(logit, x)
    ent, lp = dev(torch.full((R,), 7.0)), dev(torch.full((R,), 7.0))
    ops.onehot_ent_logp_fwd(ld, dev(x), ent, lp, unimix=U)
    check(ent, ent_ref, what=f"{what} ent")
    check(lp, lp_ref, what=f"{what} logp")
    ent.fill_(7.0)
    ops.onehot_ent_logp_fwd(ld, None, ent, None, unimix=U)
    check(ent, ent_ref, what=f"{what} ent alone")
    for use_e, use_p, acc in combos:
        _, _, gref = ref_ent_logp(logit, x, de if use_e else None, dp if use_p else None)
        dl = dev(base.clone())
        ops.onehot_ent_logp_bwd(ld, dev(x), dev(de) if use_e else None, dev(dp) if use_p else None, dl, unimix=U,
                                accumulate=acc)
        check(dl, gref + base.double() if acc else gref, what=f"{what} ent_logp_bwd e={use_e} p={use_p} acc={acc}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", ALL_D)
def test_onehot_every_group_width(ops, D, kind):
    """sample / mode / straight-through / entropy / log-prob at R = 77 (last block partly filled) for every D that
    selects another group width or leaves lanes of the group idle, on plain, saturated and edge-row logits."""
    R = 77
    g = gen(1000 + 10 * D + KINDS.index(kind))
    logit = cat_logits(R, D, kind, g)
    what = f"onehot D={D} {kind}"
    ld = run_sample_checks(ops, logit, g, what)
    run_st_bwd_checks(ops, logit, ld, g, what)
    run_ent_logp_checks(ops, logit, ld, g, what,
                        [(e, p, a) for e in (True, False) for p in (True, False) for a in (False, True)])


@pytest.mark.parametrize("R,D", [(32768 + 5, 33), (65536 + 5, 32)])
def test_onehot_grid_wrap(ops, R, D):
    """8192 blocks x 256/G rows: the second trip of the row loop at G = 64 and G = 32."""
    g = gen(R + D)
    logit = cat_logits(R, D, "randn", g)
    what = f"onehot wrap R={R} D={D}"
    ld = run_sample_checks(ops, logit, g, what)
    run_st_bwd_checks(ops, logit, ld, g, what)
    run_ent_logp_checks(ops, logit, ld, g, what, [(True, True, False), (True, True, True)])


def ref_kl(post, prior, free, dyn_scale, rep_scale, up, dt=F64):
    """networks.py:272-290 -> (kl, ent_post, ent_prior, dpost, dprior) for loss = up * sum_rows(dyn max(KL(sg p||q), free)
    + rep max(KL(p||sg q), free))."""
    p = post.to(dt).requires_grad_(True)
    q = prior.to(dt).requires_grad_(True)
    rep = O.onehot_kl(p, q.detach(), U)
    dyn = O.onehot_kl(p.detach(), q, U)
    loss = dyn_scale * torch.clip(dyn, min=free) + rep_scale * torch.clip(rep, min=free)
    (loss.sum() * up).backward()
    return rep.detach(), O.onehot_entropy(p, U).detach(), O.onehot_entropy(q, U).detach(), p.grad, q.grad


def split_point(v):
    """A `free` that some rows clear and others do not: the middle of the widest gap in the central fifth of v."""
    s = v.double().flatten().sort().values
    n = s.numel()
    if n < 4:
        return float(s.mean())
    lo, hi = int(0.4 * n), max(int(0.6 * n), int(0.4 * n) + 2)
    d = s[lo + 1:hi] - s[lo:hi - 1]
    k = int(d.argmax()) + lo
    return float(0.5 * (s[k] + s[k + 1]))


def run_kl_case(ops, rows, S, D, kind, seed):
    g = gen(seed)
    post = cat_logits(rows * S, D, kind, g).reshape(rows, S, D)
    prior = cat_logits(rows * S, D, kind, g).reshape(rows, S, D).flip(0) * 0.8
    dyn_scale, rep_scale, up = 0.5, 0.1, 1.0 / rows
    kl0 = O.onehot_kl(post.double(), prior.double(), U)
    free = split_point(kl0)
    kl_ref, ep_ref, eq_ref, dp_ref, dq_ref = ref_kl(post, prior, free, dyn_scale, rep_scale, up)
    if D > 1 and rows >= 4:
        assert 0 < (kl_ref >= free).sum().item() < rows  # the clip bites on some rows only
    what = f"kl rows={rows} S={S} D={D} {kind}"
    pd, qd = dev(post), dev(prior)
    kl, ep, eq = (dev(torch.full((rows,), 7.0)) for _ in range(3))
    ops.kl_fwd(pd, qd, kl, ep, eq, unimix=U)
    check(kl, kl_ref, what=f"{what} kl")
    check(ep, ep_ref, what=f"{what} ent_post")
    check(eq, eq_ref, what=f"{what} ent_prior")
    kl2 = dev(torch.full((rows,), 7.0))
    ops.kl_fwd(pd, qd, kl2, unimix=U)
    assert torch.equal(kl2, kl)
    bp, bq = torch.randn(rows, S, D, generator=g), torch.randn(rows, S, D, generator=g)
    for acc_p in (False, True):
        for acc_q in (False, True):
            dp, dq = dev(bp.clone()), dev(bq.clone())
            ops.kl_bwd(pd, qd, kl, dp, dq, unimix=U, free=free, dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=up,
                       acc_post=acc_p, acc_prior=acc_q)
            check(dp, dp_ref + bp.double() if acc_p else dp_ref, TOL_KL_GRAD, f"{what} dpost acc={acc_p}")
            check(dq, dq_ref + bq.double() if acc_q else dq_ref, TOL_KL_GRAD, f"{what} dprior acc={acc_q}")


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("D", ALL_D)
def test_kl_every_group_width(ops, D, S):
    """64/G groups per wave: S below that count, equal to no multiple of it, and S = 1, at every group width."""
    run_kl_case(ops, 77, S, D, "randn", 2000 + 10 * D + S)


@pytest.mark.parametrize("kind", ["wide", "edge"])
@pytest.mark.parametrize("D", ALL_D)
def test_kl_extreme_logits(ops, D, kind):
    run_kl_case(ops, 77, 5, D, kind, 2500 + 10 * D + KINDS.index(kind))


def test_kl_grid_wrap(ops):
    """4096 blocks x 4 rows: the second trip of the row loop."""
    run_kl_case(ops, 16384 + 3, 2, 5, "randn", 2999)


def first_flags(B, kind, g):
    if kind == "zeros":
        return torch.zeros(B)
    if kind == "ones":
        return torch.ones(B)
    f = (torch.rand(B, generator=g) > 0.6).float()
    f[0], f[B - 1] = 1.0, 0.0
    return f


def run_obs_carry_case(ops, B, S, D, De, first_kind, seed, pad=0):
    g = gen(seed)
    SD = S * D
    first = first_flags(B, first_kind, g)
    dsin_w = torch.randn(B, SD + pad, generator=g)
    ddin_w = torch.randn(B, De + pad, generator=g)
    dsin, ddin = dsin_w[:, :SD], ddin_w[:, :De]
    gs0, gd0 = torch.randn(B, SD, generator=g), torch.randn(B, De, generator=g)
    ds0, dd0 = torch.randn(SD, generator=g), torch.randn(De, generator=g)
    logit = cat_logits(B * S, D, "randn", g).reshape(B, S, D)
    dl0 = torch.randn(B, S, D, generator=g)
    m = first.double()[:, None]
    gs_ref = gs0.double() + dsin.double() * (1 - m)
    gd_ref = gd0.double() + ddin.double() * (1 - m)
    ds_ref = ds0.double() + (dsin.double() * m).sum(0)
    dd_ref = dd0.double() + (ddin.double() * m).sum(0)
    dl_ref = dl0.double() + ref_st_bwd(logit.reshape(B * S, D), gs_ref.reshape(B * S, D), False).reshape(B, S, D)
    gs, gd, a0, b0, dl = dev(gs0.clone()), dev(gd0.clone()), dev(ds0.clone()), dev(dd0.clone()), dev(dl0.clone())
    ops.obs_carry_st_bwd(dev(dsin_w)[:, :SD], dev(ddin_w)[:, :De], dev(first), gs, gd, a0, b0, dev(logit), dl, unimix=U)
    what = f"obs_carry B={B} S={S} D={D} De={De} first={first_kind}"
    check(gs, gs_ref, what=f"{what} gs_prev")
    check(gd, gd_ref, what=f"{what} gd_prev")
    check(a0, ds_ref, what=f"{what} dstoch0")
    check(b0, dd_ref, what=f"{what} ddeter0")
    check(dl, dl_ref, what=f"{what} dlogit_prev")


@pytest.mark.parametrize("D", ALL_D)
def test_obs_carry_st_bwd_every_group_width(ops, D):
    """B * S = 77 groups, row-strided dsin / ddin."""
    run_obs_carry_case(ops, 7, 11, D, 5, "mixed", 3000 + D, pad=3)


@pytest.mark.parametrize("B,S,D,De,first_kind", [
    (2049, 128, 3, 2, "mixed"),    # B * S > 4096 * (256 / 4): second trip of the group loop
    (2049, 1, 3, 129, "mixed"),    # B * De > 1024 * 256: second trip of the deter loop
    (2049, 1, 3, 129, "ones"),
    (2049, 1, 3, 129, "zeros"),
])
def test_obs_carry_st_bwd_grid_wrap(ops, B, S, D, De, first_kind):
    run_obs_carry_case(ops, B, S, D, De, first_kind, 3100 + S + De)


# ====================================================================================== heads (headops.hip)
STEP = 40.0 / 254.0
DISC_TARGETS = [
    0.0, 1e9, -1e9, float(O.symexp(torch.tensor(20.0))), 0.15748, -485165184.0,  # the existing edge list
    float(O.symexp(torch.tensor(-20.0))),                 # first bucket
    float(O.symexp(O.disc_buckets()[127])),               # middle bucket
    float(O.symexp(O.disc_buckets()[254])),               # last bucket
    float(O.symexp(torch.tensor(20.0 - 0.5 * STEP))),     # between the last two buckets
    float(O.symexp(O.disc_buckets()[140])), float(O.symexp(O.disc_buckets()[3])),  # exactly on a bucket
    -3.7,
]
DISC_KINDS = ["randn", "wide", "hot"]


def disc_logits(R, kind, g):
    """randn; wide: 10 randn; hot: randn with one logit of every row's first three at +80 (first / middle / last bucket)."""
    l = torch.randn(R, 255, generator=g) * (10.0 if kind == "wide" else 1.0)
    if kind == "hot":
        for r, k in zip(range(min(R, 3)), (254, 127, 0)):
            l[r, k] = 80.0
    return l


def ref_disc(logits, x, up_m, up_l, dt=F64):
    l = logits.to(dt).requires_grad_(True)
    mode = O.disc_mode(l).squeeze(-1)
    lp = O.disc_logprob(l, x.to(dt))
    (gm,) = torch.autograd.grad((mode * up_m.to(dt)).sum(), l, retain_graph=True)
    (gl,) = torch.autograd.grad((lp * up_l.to(dt)).sum(), l)
    return mode.detach(), lp.detach(), gm, gl


@pytest.mark.parametrize("kind", DISC_KINDS)
@pytest.mark.parametrize("R", [1, 3, 5, len(DISC_TARGETS), 16384 + 5])
def test_disc_head(ops, R, kind):
    """Fewer rows than the four waves of a block, every edge target, and the second trip of the 4096 x 4 row loop."""
    g = gen(4000 + R + DISC_KINDS.index(kind))
    logits = disc_logits(R, kind, g)
    x = torch.randn(R, generator=g) * 30
    T = torch.tensor(DISC_TARGETS)
    k = min(R, len(DISC_TARGETS))
    x[:k] = T.roll(-R)[:k]  # small R: another stretch of the list each
    up_m, up_l = torch.randn(R, generator=g), torch.randn(R, generator=g)
    base = torch.randn(R, 255, generator=g)
    mode_ref, lp_ref, gm_ref, gl_ref = ref_disc(logits, x, up_m, up_l)
    what = f"disc R={R} {kind}"
    ld = dev(logits)
    mode, lp = dev(torch.full((R,), 7.0)), dev(torch.full((R,), 7.0))
    ops.disc_mode_fwd(ld, mode)
    ops.disc_logprob_fwd(ld, dev(x), lp)
    check(mode, mode_ref, what=f"{what} mode")
    # the mode reaches symexp(20) = 4.9e8 on saturated rows: symlog of it (the bucket mean itself) holds every row
    check(O.symlog(mode.cpu().double()), O.symlog(mode_ref), what=f"{what} symlog(mode)")
    check(lp, lp_ref, what=f"{what} logprob")
    # Row scale of the mode's gradient up * exp(|m|) * sm_k * (b_k - m), m the bucket mean: its largest possible
    # magnitude |up| exp(|m|) (20 + |m|).  The row's own maximum will not do: on a near one-hot row the true values
    # cancel to ~0 while any fp32 evaluation keeps an error of exp(|m|) * (rounding of m), with exp(|m|) up to 4.9e8.
    m_ref = O.symlog(mode_ref)
    gm_scale = up_m.double().abs() * torch.exp(m_ref.abs()) * (20.0 + m_ref.abs())
    for acc in (False, True):
        bref = base.double() if acc else 0.0
        dl = dev(base.clone())
        ops.disc_mode_bwd(ld, dev(up_m), dl, accumulate=acc)
        check(dl, gm_ref + bref, what=f"{what} mode_bwd acc={acc}")
        check_rows(dl, gm_ref + bref, gm_scale, what=f"{what} mode_bwd by row acc={acc}")
        dl = dev(base.clone())
        ops.disc_logprob_bwd(ld, dev(x), dev(up_l), dl, accumulate=acc)
        check(dl, gl_ref + bref, what=f"{what} logprob_bwd acc={acc}")


def ref_bernoulli(l, x, up, dt=F64):
    ll = l.to(dt).requires_grad_(True)
    out = O.bernoulli_logprob(ll[:, None], x.to(dt)[:, None])
    (out * up.to(dt)).sum().backward()
    return out.detach(), ll.grad


@pytest.mark.parametrize("case", ["switch", "wrap"])
def test_bernoulli_logprob(ops, case):
    """switch: both sides of softplus's z > 20 branch and saturated sigmoids, each with x = 0 and x = 1.
    wrap: n = 2048 * 256 + 37."""
    g = gen(4100)
    if case == "switch":
        l = torch.tensor([-100.0, -20.5, -19.5, 0.0, 19.5, 20.5, 100.0]).repeat(2)
        x = torch.cat([torch.zeros(7), torch.ones(7)])
    else:
        n = 524288 + 37
        l = 3 * torch.randn(n, generator=g)
        x = (torch.rand(n, generator=g) > 0.5).float()
    n = l.numel()
    up, base = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref, gref = ref_bernoulli(l, x, up)
    out = dev(torch.full((n,), 7.0))
    ops.bernoulli_logprob_fwd(dev(l), dev(x), out)
    check(out, ref, what=f"bernoulli {case}")
    for acc in (False, True):
        dl = dev(base.clone())
        ops.bernoulli_logprob_bwd(dev(l), dev(x), dev(up), dl, accumulate=acc)
        check(dl, gref + base.double() if acc else gref, what=f"bernoulli {case} bwd acc={acc}")


def ref_symlog_mse(mode, x, up, dt=F64):
    m = mode.to(dt).requires_grad_(True)
    loss = -O.symlog_mse_logprob(m[None], x.to(dt)[None])[0]
    (loss.sum() * up).backward()
    return loss.detach(), m.grad


@pytest.mark.parametrize("R,W", [(5, 1), (5, 63), (5, 64), (5, 65), (5, 130), (1, 65), (3, 130), (16384 + 3, 65)])
def test_symlog_mse(ops, R, W):
    """W on either side of the 64-lane stride, fewer rows than waves, the second trip of the row loop, and entries
    that hit the < 1e-8 zeroing exactly (mode == symlog(x) in fp32: the squared difference is 0 or ~1e-15)."""
    g = gen(4200 + R + W)
    mode = torch.randn(R, W, generator=g)
    x = torch.randn(R, W, generator=g) * 5
    x[0, 0] = 0.0
    mode[0, W - 1] = O.symlog(x[0, W - 1])
    mode[R - 1, 0] = O.symlog(x[R - 1, 0])
    up = 0.5
    ref, gref = ref_symlog_mse(mode, x, up)
    assert gref[0, W - 1] == 0 and gref[R - 1, 0] == 0
    loss, dm = dev(torch.full((R,), 7.0)), dev(torch.full((R, W), 7.0))
    ops.symlog_mse(dev(mode), dev(x), loss, dm, upstream=up)
    check(loss, ref, what=f"symlog_mse R={R} W={W}")
    check(dm, gref, what=f"symlog_mse R={R} W={W} dmode")
    assert dm[0, W - 1].item() == 0.0 and dm[R - 1, 0].item() == 0.0
    loss2 = dev(torch.full((R,), 7.0))
    ops.symlog_mse(dev(mode), dev(x), loss2)
    assert torch.equal(loss2, loss)


@pytest.mark.parametrize("n", [1, 255, 524288 + 37])
def test_symlog(ops, n):
    g = gen(4300 + n)
    x = torch.randn(n, generator=g) * 50
    x[0] = 0.0
    if n > 4:
        x[1:5] = torch.tensor([1e9, -1e9, 1e-6, -1e-6])
    y = dev(torch.full((n,), 7.0))
    ops.symlog(dev(x), y)
    check(y, O.symlog(x.double()), what=f"symlog n={n}")


@pytest.mark.parametrize("n", [5, 524288 + 37])
def test_tanh(ops, n):
    """tanh_fwd / tanh_bwd (the backward takes y): saturated arguments and the second trip of the 2048 x 256 loop."""
    g = gen(4350 + n)
    x = torch.randn(n, generator=g) * 2
    x[:5] = torch.tensor([0.0, 30.0, -30.0, 1e-4, -9.5])
    dy, base = torch.randn(n, generator=g), torch.randn(n, generator=g)
    xr = x.double().requires_grad_(True)
    yr = torch.tanh(xr)
    yr.backward(dy.double())
    y = dev(torch.full((n,), 7.0))
    ops.tanh_fwd(dev(x), y)
    check(y, yr, what=f"tanh n={n}")
    for acc in (False, True):
        dx = dev(base.clone())
        ops.tanh_bwd(y, dev(dy), dx, accumulate=acc)
        check(dx, xr.grad + base.double() if acc else xr.grad, what=f"tanh_bwd n={n} acc={acc}")


@pytest.mark.parametrize("B,T,k", [(3, 5, 1), (7, 3, 11), (17, 33, 941)])
def test_transpose01(ops, B, T, k):
    """[B,T,k] -> [T,B,k], an exact copy; 17 * 33 * 941 > 2048 * 256 takes the second trip of the loop."""
    x = torch.randn(B, T, k, generator=gen(4360 + k))
    y = dev(torch.full((T, B, k), 7.0))
    ops.transpose01(dev(x), y)
    assert torch.equal(y.cpu(), x.transpose(0, 1).contiguous())


def ref_mse_image(recon, img, up, perm, dt=F64):
    """recon image n' = t * B + b pairs with replay image b * T + t when perm = (B, T)."""
    n, P = recon.shape
    r = recon.to(dt).requires_grad_(True)
    t = img.to(dt) / 255.0
    if perm is not None:
        B, T = perm
        t = t.reshape(B, T, P).transpose(0, 1).reshape(n, P)
    loss = ((r - t) ** 2).sum(-1)
    (loss.sum() * up).backward()
    return loss.detach(), r.grad


@pytest.mark.parametrize("perm", [None, (2, 3)])
@pytest.mark.parametrize("pixels", [4, 1020, 1028, 12288])
def test_mse_image(ops, pixels, perm):
    """One float4 for one thread, 255 and 257 float4 per 256-thread block, and a 64 x 64 x 3 image."""
    g = gen(4400 + pixels)
    n = 6
    img = torch.randint(0, 256, (n, pixels), generator=g, dtype=torch.uint8)
    recon = torch.rand(n, pixels, generator=g) * 1.2 - 0.1
    up = 0.25
    ref, gref = ref_mse_image(recon, img, up, perm)
    loss, dr = dev(torch.full((n,), 7.0)), dev(torch.full((n, pixels), 7.0))
    ops.mse_image(dev(recon), dev(img), loss, dr, upstream=up, perm=perm)
    check(loss, ref, what=f"mse_image P={pixels} perm={perm}")
    check(dr, gref, what=f"mse_image P={pixels} perm={perm} drecon")
    loss2 = dev(torch.full((n,), 7.0))
    ops.mse_image(dev(recon), dev(img), loss2, None, perm=perm)
    assert torch.equal(loss2, loss)


# ====================================================================================== behaviour (headops.hip)
MIN_STD, MAX_STD = 0.1, 1.0
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))


def ref_actor_normal(mr, sr, eps, fixed, da=None, de=None, dl=None, logp_of_sample=False, dt=F64):
    """networks.py:693-700 / tools.ContDist with absmax = 1 -> (action, entropy, logp(fixed), dmean_raw, dstd_raw)."""
    m = mr.to(dt).requires_grad_(True)
    s = sr.to(dt).requires_grad_(True)
    mean = torch.tanh(m)
    std = (MAX_STD - MIN_STD) * torch.sigmoid(s + 2.0) + MIN_STD
    pre = mean + std * eps.to(dt)
    act = pre * (1.0 / torch.clip(pre.abs(), min=1.0)).detach()
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).sum(-1)
    a = act if logp_of_sample else fixed.to(dt)
    lp = (-((a - mean) ** 2) / (2 * std ** 2) - torch.log(std) - LOG_SQRT_2PI).sum(-1)
    tot = (m * 0).sum() + (s * 0).sum()
    if da is not None:
        tot = tot + (act * da.to(dt)).sum()
    if de is not None:
        tot = tot + (ent * de.to(dt)).sum()
    if dl is not None:
        tot = tot + (lp * dl.to(dt)).sum()
    gm, gs = torch.autograd.grad(tot, (m, s))
    return act.detach(), ent.detach(), lp.detach(), gm, gs


def actor_inputs(M, A, kind, g):
    mr = torch.randn(M, A, generator=g)
    sr = torch.randn(M, A, generator=g)
    eps = torch.randn(M, A, generator=g) * 1.5
    if kind == "sat":
        # std saturated to min_std / max_std, and |mean + std eps| a hair on either side of the absmax clip at 1
        sr = torch.where(torch.rand(M, A, generator=g) > 0.5, 30.0, -30.0)
        std = torch.where(sr > 0, MAX_STD, MIN_STD)
        side = torch.where(torch.rand(M, A, generator=g) > 0.5, 1.0, -1.0)
        mag = 1.0 + torch.tensor([-0.3, -1e-3, 1e-3, 0.3, 2.0]).repeat(M * A // 5 + 1)[:M * A].reshape(M, A)
        eps = (side * mag - torch.tanh(mr)) / std
    return mr, sr, eps


@pytest.mark.parametrize("kind", ["randn", "sat"])
@pytest.mark.parametrize("M,A", [(77, 1), (77, 6), (77, 17), (524288 + 5, 1)])
def test_actor_normal(ops, M, A, kind):
    """A = 1 / 6 / 17, the second trip of the 2048 x 256 row loop, std at both ends of its range, |pre-clip action| on
    both sides of 1; every None-combination of the three upstreams, log-prob of a constant and of the sample."""
    g = gen(5000 + M + A + (kind == "sat"))
    mr, sr, eps = actor_inputs(M, A, kind, g)
    da, de, dl = torch.randn(M, A, generator=g), torch.randn(M, generator=g), torch.randn(M, generator=g)
    act_ref, ent_ref, _, _, _ = ref_actor_normal(mr, sr, eps, eps)
    if kind == "sat":
        pre = torch.tanh(mr.double()) + ((MAX_STD - MIN_STD) * torch.sigmoid(sr.double() + 2) + MIN_STD) * eps.double()
        assert (pre.abs() > 1).any() and (pre.abs() < 1).any()
    fixed = (act_ref + 0.1).float()
    _, _, lp_ref, _, _ = ref_actor_normal(mr, sr, eps, fixed)
    what = f"actor_normal M={M} A={A} {kind}"
    mrd, srd, epd, fxd = dev(mr), dev(sr), dev(eps), dev(fixed)
    action, ent, lp = dev(torch.full((M, A), 7.0)), dev(torch.full((M,), 7.0)), dev(torch.full((M,), 7.0))
    ops.actor_normal_fwd(mrd, srd, epd, action, ent, min_std=MIN_STD, max_std=MAX_STD)
    ops.actor_normal_logp(mrd, srd, fxd, lp, min_std=MIN_STD, max_std=MAX_STD)
    check(action, act_ref, what=f"{what} action")
    check(ent, ent_ref, what=f"{what} entropy")
    check(lp, lp_ref, what=f"{what} logp")
    ent.fill_(7.0)
    ops.actor_normal_fwd(mrd, srd, None, None, ent, min_std=MIN_STD, max_std=MAX_STD)  # entropy alone: no eps needed
    check(ent, ent_ref, what=f"{what} entropy alone")
    act32 = action  # the log-prob of the sample is taken of the action the kernel itself produced
    combos = [(a, e, l, s) for a in (True, False) for e in (True, False) for l in (True, False)
              for s in ((False, True) if l else (False,))]
    if M > 1000:
        combos = [(True, True, True, False), (True, True, True, True)]
    for use_a, use_e, use_l, of_sample in combos:
        _, _, _, gm_ref, gs_ref = ref_actor_normal(mr, sr, eps, fixed, da if use_a else None, de if use_e else None,
                                                   dl if use_l else None, of_sample)
        dm, ds = dev(torch.full((M, A), 7.0)), dev(torch.full((M, A), 7.0))
        ops.actor_normal_bwd(mrd, srd, dm, ds, eps=epd, action=act32 if of_sample else fxd,
                             daction=dev(da) if use_a else None, dent=dev(de) if use_e else None,
                             dlogp=dev(dl) if use_l else None, min_std=MIN_STD, max_std=MAX_STD,
                             logp_of_sample=of_sample)
        tag = f"{what} bwd a={use_a} e={use_e} l={use_l} sample={of_sample}"
        check(dm, gm_ref, what=f"{tag} dmean_raw")
        check(ds, gs_ref, what=f"{tag} dstd_raw")


def ref_lambda_return(reward, value, cl, dtarget, gamma, lam, dt=F64):
    """models.py:620-638 + tools.lambda_return -> (target [H-1,N], weights [H,N], disc [H,N], dreward, dcont_logit)."""
    r = reward.to(dt).requires_grad_(True)
    c = cl.to(dt).requires_grad_(True)
    disc = gamma * torch.sigmoid(c)
    tgt = O.lambda_return(r, value.to(dt), disc, lam)
    w = torch.cumprod(torch.cat([torch.ones_like(disc[:1]), disc[:-1]], 0), 0)
    gr, gc = torch.autograd.grad((tgt * dtarget.to(dt)).sum(), (r, c), allow_unused=True)
    gr = torch.zeros_like(r) if gr is None else gr
    gc = torch.zeros_like(c) if gc is None else gc
    return tgt.detach(), w.detach(), disc.detach(), gr, gc


@pytest.mark.parametrize("gamma", [1.0, 0.997])
@pytest.mark.parametrize("H,N", [(2, 77), (3, 77), (16, 77), (3, 524288 + 37)])
def test_lambda_return(ops, H, N, gamma):
    """H = 2 (bootstrap only), 3, 16; the second trip of the column loop; continue-logits of +-50 in the discount
    product; gamma = 1.0 as tools.lambda_return calls it; with and without the disc output."""
    g = gen(5100 + H + N)
    lam = 0.95
    reward = torch.randn(H, N, generator=g)
    value = torch.randn(H, N, generator=g) * 3
    cl = 2 * torch.randn(H, N, generator=g)
    cl[:, 0], cl[:, 1] = 50.0, -50.0
    cl[H - 1, 2], cl[0, 3], cl[1, 4] = -50.0, -50.0, 50.0
    dtg = torch.randn(H - 1, N, generator=g)
    tgt_ref, w_ref, d_ref, gr_ref, gc_ref = ref_lambda_return(reward, value, cl, dtg, gamma, lam)
    what = f"lambda_return H={H} N={N} gamma={gamma}"
    rd, vd, cd = dev(reward), dev(value), dev(cl)
    tgt, w, d = dev(torch.full((H - 1, N), 7.0)), dev(torch.full((H, N), 7.0)), dev(torch.full((H, N), 7.0))
    ops.lambda_return_fwd(rd, vd, cd, tgt, w, d, gamma=gamma, lam=lam)
    check(tgt, tgt_ref, what=f"{what} target")
    check(w, w_ref, what=f"{what} weights")
    check(d, d_ref, what=f"{what} disc")
    tgt2, w2 = dev(torch.full((H - 1, N), 7.0)), dev(torch.full((H, N), 7.0))
    ops.lambda_return_fwd(rd, vd, cd, tgt2, w2, None, gamma=gamma, lam=lam)
    assert torch.equal(tgt2, tgt) and torch.equal(w2, w)
    dr, dc = dev(torch.full((H, N), 7.0)), dev(torch.full((H, N), 7.0))
    ops.lambda_return_bwd(dev(dtg), vd, cd, tgt, dr, dc, gamma=gamma, lam=lam)
    check(dr, gr_ref, what=f"{what} dreward")
    check(dc, gc_ref, what=f"{what} dcont_logit")
    assert not dr[0].any() and not dc[0].any()  # reward_0 and cont_0 reach no target


def ref_actor_loss(target, value, weights, ent, logp, ema, loss0, ent_coef, mode, mix, dt=F64):
    """models.py:406-407 and 640-681: -> (loss0 + mean loss, dtarget [H-1,N], dlogp [H,N], dent [H,N])."""
    t = target.to(dt).requires_grad_(True)
    e = ent.to(dt).requires_grad_(True)
    lp = logp.to(dt).requires_grad_(True)
    base, w = value.to(dt)[:-1], weights.to(dt)[:-1]
    offset = ema.to(dt)[0]
    scale = torch.clip(ema.to(dt)[1] - ema.to(dt)[0], min=1.0)
    adv = (t - offset) / scale - (base - offset) / scale
    if mode == 0:
        actor_target = adv
    else:
        actor_target = lp[:-1] * (t - base).detach()
        if mode == 2:
            actor_target = mix * t + (1 - mix) * actor_target
    loss = torch.mean(-w * actor_target - ent_coef * e[:-1])
    gt, glp, ge = torch.autograd.grad(loss, (t, lp, e), allow_unused=True)
    gt = torch.zeros_like(t) if gt is None else gt
    glp = torch.zeros_like(lp) if glp is None else glp
    return loss.detach() + loss0, gt, glp, ge


@pytest.mark.parametrize("ema", [(0.2, 0.7), (-1.0, 4.0)])
@pytest.mark.parametrize("mode,mix", [(0, 0.0), (1, 0.0), (2, 0.0), (2, 0.3), (2, 1.0)])
@pytest.mark.parametrize("H,N", [(2, 77), (16, 77)])
def test_actor_loss(ops, H, N, mode, mix, ema):
    """The three objectives of imag_gradient ('dynamics', 'reinforce', 'both' with its mix), the EMA scale below and
    above the max(., 1), H * N no multiple of 256, a non-zero loss accumulator, and the zero last row of dent / dlogp."""
    g = gen(5200 + H + 10 * mode + int(10 * mix))
    target = torch.randn(H - 1, N, generator=g) * 3
    value = torch.randn(H, N, generator=g) * 3
    weights = torch.rand(H, N, generator=g)
    ent = torch.randn(H, N, generator=g)
    logp = torch.randn(H, N, generator=g) * 2
    ema_t = torch.tensor(ema)
    ent_coef, loss0 = 0.3, 0.25
    loss_ref, gt_ref, glp_ref, ge_ref = ref_actor_loss(target, value, weights, ent, logp, ema_t, loss0, ent_coef, mode, mix)
    what = f"actor_loss H={H} mode={mode} mix={mix} ema={ema}"
    loss = dev(torch.tensor([loss0]))
    dtg = dev(torch.full((H - 1, N), 7.0)) if mode != 1 else None
    dlp = dev(torch.full((H, N), 7.0)) if mode != 0 else None
    de = dev(torch.full((H, N), 7.0))
    ops.actor_loss(dev(target), dev(value), dev(weights), dev(ent), dev(ema_t), loss, de, dtarget=dtg,
                   logp=dev(logp) if mode != 0 else None, dlogp=dlp, entropy_coef=ent_coef, mode=mode, mix=mix)
    check(loss, loss_ref.reshape(1), what=f"{what} loss")
    # the gradients of a mean over (H - 1) N entries are ~1e-3: held relative to their own maximum, not to 1
    check(de, ge_ref, what=f"{what} dent", floor=0.0)
    assert not de[H - 1].any()
    if dtg is not None:
        check(dtg, gt_ref, what=f"{what} dtarget", floor=0.0)
    else:
        assert not gt_ref.any()
    if dlp is not None:
        check(dlp, glp_ref, what=f"{what} dlogp", floor=0.0)
        assert not dlp[H - 1].any()
    else:
        assert not glp_ref.any()


@pytest.mark.parametrize("clip_min", [None, 0.0, 1.0])
@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 1024 * 512 + 9])
def test_dot_accumulate(ops, n, with_w, clip_min):
    """out += scale * sum(max(x, clip_min) * w): one thread, either side of a block, the second trip of the 512 x 1024
    loop; a non-zero accumulator and scale != 1."""
    g = gen(5300 + n)
    x = torch.randn(n, generator=g) * 2
    w = torch.randn(n, generator=g) if with_w else None
    scale, out0 = 0.37, 2.5
    v = x.double() if clip_min is None else torch.clip(x.double(), min=clip_min)
    ref = out0 + scale * (v * w.double() if with_w else v).sum()
    out = dev(torch.tensor([out0]))
    ops.dot_accumulate(dev(x), out, w=dev(w) if with_w else None, clip_min=clip_min, scale=scale)
    check(out, ref.reshape(1), what=f"dot_accumulate n={n} w={with_w} clip={clip_min}")


@pytest.mark.parametrize("n", [1, 255, 2048 * 256 + 7])
def test_scale_neg_axpby(ops, n):
    """scale_neg is one fp32 product: equal to the rounded float64 product.  axpby is a x + b y in fp32: every element
    must equal one of the three results an fp32 evaluation can give, each computed in float64 and rounded once --
    round(round(a x) + round(b y)), fma(a, x, round(b y)) or fma(b, y, round(a x)).  (a x and b y are exact in float64;
    all three lie within 1 ulp of the exact sum unless the addends cancel.)"""
    g = gen(5400 + n)
    w = torch.randn(n, generator=g)
    s = float(torch.tensor(1.0 / 1387.0))  # the fp32 value the launcher receives
    out = dev(torch.full((n,), 7.0))
    ops.scale_neg(dev(w), out, s)
    assert torch.equal(out.cpu(), (-(w.double() * s)).float())
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = float(torch.tensor(0.02)), float(torch.tensor(0.98))
    ax, by = a * x.double(), b * y.double()
    ref = ax + by
    yd = dev(y.clone())
    ops.axpby(dev(x), yd, a, b)
    rax, rby = ax.float().double(), by.float().double()
    cands = [(rax + rby).float(), (ax + rby).float(), (rax + by).float()]
    got = yd.cpu()
    hit = [got == c for c in cands]
    print(f"axpby n={n}: unfused {int(hit[0].sum())} fma(a,x,.) {int(hit[1].sum())} fma(b,y,.) {int(hit[2].sum())} of {n}")
    assert (hit[0] | hit[1] | hit[2]).all()
    assert hit[0].all() or hit[1].all() or hit[2].all()  # one evaluation order for the whole tensor


@pytest.mark.parametrize("lens", [(5,), (1,), (7, 1, 300), (3, 1, 1025, 2, 64, 9), (300000, 1, 5)])
def test_concat_flat(ops, lens):
    """1, 3 and 6 parts, a part of length 1, and more than 1024 x 256 elements: an exact copy."""
    g = gen(5500 + len(lens))
    parts = [torch.randn(k, generator=g) for k in lens]
    dst = dev(torch.full((sum(lens),), 7.0))
    ops.concat_flat([dev(p) for p in parts], dst)
    assert torch.equal(dst.cpu(), torch.cat(parts))


@pytest.mark.parametrize("first_kind", ["zeros", "ones", "mixed"])
def test_reset_blend_grid_wrap(ops, first_kind):
    """B * n > 2048 * 256 (forward) and n > 2048 * 256 (backward): the second trip of both loops.  The blend with a
    0 / 1 flag is exact."""
    g = gen(5600)
    B, n = 3, 524288 + 37
    first = first_flags(B, first_kind, g)
    x, init, go = torch.randn(B, n, generator=g), torch.randn(n, generator=g), torch.randn(B, n, generator=g)
    di0 = torch.randn(n, generator=g)
    m = first[:, None]
    out = dev(torch.full((B, n), 7.0))
    ops.reset_blend(dev(x), dev(init), dev(first), out)
    assert torch.equal(out.cpu(), x * (1 - m) + init[None] * m)
    dx, di = dev(torch.full((B, n), 7.0)), dev(di0.clone())
    ops.reset_blend_bwd(dev(go), dev(first), dx, di)
    assert torch.equal(dx.cpu(), go * (1 - m))
    check(di, di0.double() + (go.double() * m.double()).sum(0), what=f"reset_blend_bwd dinit first={first_kind}")


@pytest.mark.parametrize("first_kind", ["zeros", "ones", "mixed"])
def test_obs_blend_grid_wrap(ops, first_kind):
    """B * (SD + De + A) and B * (SD + De) above 1024 * 256: the second trip of obs_blend and obs_blend_bwd."""
    g = gen(5700)
    B, SD, De, A = 33, 4000, 4001, 7
    first = first_flags(B, first_kind, g)
    m = first[:, None]
    ps, pd, ac = torch.randn(B, SD, generator=g), torch.randn(B, De, generator=g), torch.randn(B, A, generator=g)
    s0, d0 = torch.randn(SD, generator=g), torch.randn(De, generator=g)
    os_, od_, oa_ = dev(torch.full((B, SD), 7.0)), dev(torch.full((B, De), 7.0)), dev(torch.full((B, A), 7.0))
    ops.obs_blend(dev(ps), dev(s0), dev(pd), dev(d0), dev(ac), dev(first), os_, od_, oa_)
    assert torch.equal(os_.cpu(), ps * (1 - m) + s0 * m)
    assert torch.equal(od_.cpu(), pd * (1 - m) + d0 * m)
    assert torch.equal(oa_.cpu(), ac * (1 - m))
    if first_kind == "ones":  # the first step of a scan: no previous state
        os_.fill_(7.0), od_.fill_(7.0), oa_.fill_(7.0)
        ops.obs_blend(None, dev(s0), None, dev(d0), dev(ac), dev(first), os_, od_, oa_)
        assert torch.equal(os_.cpu(), s0.expand(B, SD)) and torch.equal(od_.cpu(), d0.expand(B, De))
        assert not oa_.any()
    gs0, gd0 = torch.randn(B, SD, generator=g), torch.randn(B, De, generator=g)
    dsn, ddn = torch.randn(B, SD, generator=g), torch.randn(B, De, generator=g)
    a00, b00 = torch.randn(SD, generator=g), torch.randn(De, generator=g)
    gs, gd, a0, b0 = dev(gs0.clone()), dev(gd0.clone()), dev(a00.clone()), dev(b00.clone())
    ops.obs_blend_bwd(dev(dsn), dev(ddn), dev(first), gs, gd, a0, b0)
    md = m.double()
    what = f"obs_blend_bwd first={first_kind}"
    check(gs, gs0.double() + dsn.double() * (1 - md), what=f"{what} gs_prev")
    check(gd, gd0.double() + ddn.double() * (1 - md), what=f"{what} gd_prev")
    check(a0, a00.double() + (dsn.double() * md).sum(0), what=f"{what} dstoch0")
    check(b0, b00.double() + (ddn.double() * md).sum(0), what=f"{what} ddeter0")


# ====================================================================================== optimizer (optim.hip)
ADAM_NS = [1, 5, 100003, 2048 * 256 + 7]


@pytest.mark.parametrize("n", ADAM_NS)
def test_sumsq(ops, n):
    """out += sum x^2 by atomics and in the fixed order, from a non-zero accumulator; float4 body and scalar tail."""
    g = gen(6000 + n)
    x = torch.randn(n, generator=g) * 3
    ref = 1.25 + (x.double() ** 2).sum()
    xd = dev(x)
    out = dev(torch.tensor([1.25]))
    ops.sumsq_accumulate(xd, out)
    check(out, ref.reshape(1), TOL_SUMSQ, f"sumsq_accumulate n={n}", floor=0.0)
    out = dev(torch.tensor([1.25]))
    ops.sumsq_ordered(xd, out, dev(torch.zeros(1024)))
    check(out, ref.reshape(1), TOL_SUMSQ, f"sumsq_ordered n={n}", floor=0.0)
    out = dev(torch.tensor([1.25]))
    ops.sumsq_ordered(xd, out, dev(torch.zeros(3)))  # a short scratch caps the grid
    check(out, ref.reshape(1), TOL_SUMSQ, f"sumsq_ordered n={n} (3 partials)", floor=0.0)


def ref_adam_step(p, g, m, v, step, *, lr, eps, clip, wd, gscale, b1=0.9, b2=0.999):
    """tools.Optimizer.__call__ (tools.py:760-783) around torch.optim.Adam, in float64 and out of place: weight decay
    on the parameters, clip_grad_norm_ on the scaled gradient, then the Adam step.  -> (p, m, v, step, scaled norm)."""
    if wd:
        p = p * (1 - wd)
    norm = (g ** 2).sum().sqrt() * gscale
    coef = torch.clamp(clip / (norm + 1e-6), max=1.0) if clip else 1.0
    g = g * gscale * coef
    step = step + 1
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    p = p - (lr / (1 - b1 ** step)) * m / denom
    return p, m, v, step, norm


def adam_grads(n, steps, big_steps, g):
    """Small gradients (norm far below the clip of 100) except on big_steps (norm above it for every n >= 1)."""
    return [torch.randn(n, generator=g) * 0.01 + (300.0 if it in big_steps else 0.0) for it in range(steps)]


def run_adam(ops, p0, m0, v0, step0, grads, *, lr, eps, clip, wd, gscale, ref=True, ordered=True, what="adam"):
    """One kernel step per gradient; with ref, a float64 optimizer runs beside it from the same start (its own
    trajectory, never re-synchronised) and parameters and moments are compared after every step.  -> final fp32
    parameters."""
    n = p0.numel()
    pd, md, vd = dev(p0.clone()), dev(m0.clone()), dev(v0.clone())
    state = dev(torch.tensor([float(step0), 0.0, -1.0, 0.0]))
    partial = dev(torch.zeros(1024))
    p64, m64, v64, step = p0.double(), m0.double(), v0.double(), step0
    for it, grad in enumerate(grads):
        gd = dev(grad)
        if ordered and it % 2:
            ops.sumsq_ordered(gd, state[1:2], partial)
        else:
            ops.sumsq_accumulate(gd, state[1:2])
        ops.adam_step(pd, gd, md, vd, state, lr=lr, eps=eps, clip=clip, weight_decay=wd, grad_scale=gscale)
        st = state.cpu()
        assert st[0].item() == step0 + it + 1 and st[1].item() == 0.0
        if not ref:
            continue
        p64, m64, v64, step, norm = ref_adam_step(p64, grad.double(), m64, v64, step, lr=lr, eps=eps, clip=clip, wd=wd,
                                                  gscale=gscale)
        print(f"{what} it {it}: norm {st[2].item():.6e} ref {norm.item():.6e}")
        assert abs(st[2].item() - norm.item()) <= 1e-4 * norm.item(), f"{what} it {it}: scaled norm"
        check(pd, p64, TOL_ADAM, f"{what} it {it} param")
        # the moments are ~1e-3 and ~1e-7 on the small-gradient steps: each against its own maximum
        check(md, m64, TOL_ADAM, f"{what} it {it} exp_avg", floor=0.0)
        check(vd, v64, TOL_ADAM, f"{what} it {it} exp_avg_sq", floor=0.0)
    return pd.cpu()


@pytest.mark.parametrize("gscale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [0.0, 100.0])
@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_step(ops, n, clip, wd, gscale):
    """Decay -> clip on the scaled norm -> Adam, five steps, gradients below and above the clip.  With grad_scale the
    raw gradients are 1 / grad_scale times larger, as the summed gradients of 8 data-parallel ranks are."""
    g = gen(6100 + n)
    p0 = torch.randn(n, generator=g)
    z = torch.zeros(n)
    grads = [gr / gscale for gr in adam_grads(n, 5, (1, 3), g)]
    run_adam(ops, p0, z, z, 0, grads, lr=1e-2, eps=1e-8, clip=clip, wd=wd, gscale=gscale,
             what=f"adam n={n} clip={clip} wd={wd} gscale={gscale}")


@pytest.mark.parametrize("clip", [0.0, 100.0])
@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_grad_scale_is_exact(ops, n, clip):
    """grad_scale = 1/8 on gradients 8 g (an exactly representable multiple) gives bit for bit the parameters of
    grad_scale = 1 on g while the clip does not bite: what the data-parallel path assumes of the summed gradient."""
    g = gen(6200 + n)
    p0 = torch.randn(n, generator=g)
    z = torch.zeros(n)
    grads = adam_grads(n, 5, (), g)
    kw = dict(lr=1e-2, eps=1e-8, clip=clip, wd=0.01, ref=False)
    pa = run_adam(ops, p0, z, z, 0, grads, gscale=1.0, **kw)
    pb = run_adam(ops, p0, z, z, 0, [8.0 * gr for gr in grads], gscale=0.125, **kw)
    assert torch.equal(pa, pb)
    assert not torch.equal(pa, p0)


@pytest.mark.parametrize("n", [5, 100003])
def test_adam_resumes_from_a_checkpoint(ops, n):
    """state[0] = 999 with non-zero moments, as _BucketAdam.load_state_dict leaves them: the bias corrections use 1000."""
    g = gen(6300 + n)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.01
    v0 = torch.rand(n, generator=g) * 1e-4
    grads = adam_grads(n, 5, (1, 3), g)
    run_adam(ops, p0, m0, v0, 999, grads, lr=1e-2, eps=1e-8, clip=100.0, wd=0.01, gscale=1.0, what=f"adam resume n={n}")
