"""Per-kernel parity of csrc/gaussops.hip (continuous Gaussian latents, dyn_discrete: 0) against torch.distributions
in float64 on the CPU: the stat-layer head with its reparameterised sample, its backward, the KL / entropies and their
backward.

Bars (README "correctness" row): outputs 1e-4 of max(1, |ref|max); gradients 5e-6 of the reference tensor's max.
"""
import itertools

import pytest
import torch
import torch.distributions as torchd
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4
GRAD_TOL = 5e-6

MEAN_ACTS = ["none", "tanh5"]
STD_ACTS = ["softplus", "abs", "sigmoid", "sigmoid2", "identity"]  # identity: the raw value already is the std
S_LIST = [1, 8, 30, 32, 64, 200]
M_LIST = [1, 16, 1024, 15360]


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def assert_close(got, ref, tol=TOL, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"{what}: max err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def assert_grad_close(got, ref, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = ref.abs().max().item() if ref.numel() else 0.0
    print(f"{what}: max err {err:.3e} tensor max {scale:.3e}")
    assert err <= GRAD_TOL * scale, f"{what}: max err {err:.3e} vs tensor max {scale:.3e}"


def ref_stats(raw, S, mean_act, std_act, min_std):
    """RSSM._suff_stats_layer of the reference (continuous branch) on a float64 tensor."""
    mean, std = torch.split(raw, [S] * 2, -1)
    mean = {"none": lambda: mean, "tanh5": lambda: 5.0 * torch.tanh(mean / 5.0)}[mean_act]()
    std = {"softplus": lambda: F.softplus(std), "abs": lambda: torch.abs(std + 1),
           "sigmoid": lambda: torch.sigmoid(std), "sigmoid2": lambda: 2 * torch.sigmoid(std / 2),
           "identity": lambda: std}[std_act]()
    return mean, std + min_std


def ref_rsample(mean, std, eps, monkeypatch):
    """Normal(mean, std).rsample() with the N(0,1) draw replaced by `eps` (float64)."""
    with monkeypatch.context() as mp:
        mp.setattr(torchd.normal, "_standard_normal", lambda shape, dtype, device: eps.reshape(tuple(shape)))
        return torchd.Independent(torchd.Normal(mean, std), 1).rsample()


def head_inputs(M, S, seed=0):
    g = torch.Generator().manual_seed(1000 * S + M + seed)
    raw = 2.0 * torch.randn(M, 2 * S, generator=g)
    eps = torch.randn(M, S, generator=g)
    up = [torch.randn(M, S, generator=g) for _ in range(3)]
    return raw, eps, up


@pytest.mark.parametrize("mean_act,std_act", list(itertools.product(MEAN_ACTS, STD_ACTS)))
@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("M", M_LIST)
def test_head_fwd_bwd(ops, monkeypatch, M, S, mean_act, std_act):
    min_std = 0.1
    raw, eps, (gs, gm, gd) = head_inputs(M, S)
    if std_act == "identity":
        raw[:, S:] = raw[:, S:].abs() + 0.05  # a standard deviation
    r64 = raw.double().requires_grad_(True)
    mean_r, std_r = ref_stats(r64, S, mean_act, std_act, min_std)
    stoch_r = ref_rsample(mean_r, std_r, eps.double(), monkeypatch)
    ((stoch_r * gs.double()).sum() + (mean_r * gm.double()).sum() + (std_r * gd.double()).sum()).backward()

    mk = lambda *s: torch.full(s, float("nan"), device="cuda")
    mean, std, stoch, eps_out = mk(M, S), mk(M, S), mk(M, S), mk(M, S)
    rd = raw.cuda()
    ops.gauss_head_fwd(rd, stoch, mean, std, eps=eps.cuda(), eps_out=eps_out, mean_act=mean_act, std_act=std_act,
                       min_std=min_std)
    assert_close(mean, mean_r, what="mean")
    assert_close(std, std_r, what="std")
    assert_close(stoch, stoch_r, what="stoch")
    assert torch.equal(eps_out.cpu(), eps)
    draw = mk(M, 2 * S)
    ops.gauss_head_bwd(rd, draw, dstoch=gs.cuda(), dmean=gm.cuda(), dstd=gd.cuda(), eps=eps_out, mean_act=mean_act,
                       std_act=std_act)
    assert_grad_close(draw, r64.grad, what="draw")


@pytest.mark.parametrize("mean_act,std_act", [("none", "sigmoid2"), ("tanh5", "softplus")])
@pytest.mark.parametrize("M,S", [(16, 8), (1024, 30), (7, 200)])
def test_head_mode_form(ops, M, S, mean_act, std_act):
    """mode: stoch = mean, nothing is drawn, and the backward has no eps term."""
    raw, eps, (gs, gm, gd) = head_inputs(M, S, seed=1)
    r64 = raw.double().requires_grad_(True)
    mean_r, std_r = ref_stats(r64, S, mean_act, std_act, 0.1)
    stoch_r = torchd.Independent(torchd.Normal(mean_r, std_r), 1).mean  # tools.ContDist.mode of the reference
    ((stoch_r * gs.double()).sum() + (std_r * gd.double()).sum()).backward()
    rd = raw.cuda()
    mean, std, stoch = (torch.empty(M, S, device="cuda") for _ in range(3))
    eps_out = torch.full((M, S), 7.0, device="cuda")
    ops.gauss_head_fwd(rd, stoch, mean, std, eps_out=eps_out, mean_act=mean_act, std_act=std_act, min_std=0.1, mode=True)
    assert_close(stoch, stoch_r, what="stoch")
    assert torch.equal(stoch, mean)
    assert_close(std, std_r, what="std")
    assert bool((eps_out == 7.0).all())
    draw = torch.empty(M, 2 * S, device="cuda")
    # eps given or not: the mode form ignores it
    ops.gauss_head_bwd(rd, draw, dstoch=gs.cuda(), dstd=gd.cuda(), eps=eps.cuda(), mean_act=mean_act, std_act=std_act,
                       mode=True)
    assert_grad_close(draw, r64.grad, what="draw")
    draw2 = torch.empty(M, 2 * S, device="cuda")
    ops.gauss_head_bwd(rd, draw2, dstoch=gs.cuda(), dstd=gd.cuda(), mean_act=mean_act, std_act=std_act, mode=True)
    assert torch.equal(draw, draw2)


NULL_COMBOS = [c for c in itertools.product([False, True], repeat=3) if any(c)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("use_s,use_m,use_d", NULL_COMBOS)
def test_head_bwd_null_gradients_and_accumulate(ops, monkeypatch, use_s, use_m, use_d, accumulate):
    M, S, mean_act, std_act = 48, 30, "tanh5", "sigmoid2"
    raw, eps, (gs, gm, gd) = head_inputs(M, S, seed=2)
    r64 = raw.double().requires_grad_(True)
    mean_r, std_r = ref_stats(r64, S, mean_act, std_act, 0.1)
    stoch_r = ref_rsample(mean_r, std_r, eps.double(), monkeypatch)
    loss = 0.0
    if use_s:
        loss = loss + (stoch_r * gs.double()).sum()
    if use_m:
        loss = loss + (mean_r * gm.double()).sum()
    if use_d:
        loss = loss + (std_r * gd.double()).sum()
    loss.backward()
    base = torch.randn(M, 2 * S, generator=torch.Generator().manual_seed(5))
    draw = base.cuda() if accumulate else torch.full((M, 2 * S), float("nan"), device="cuda")
    ops.gauss_head_bwd(raw.cuda(), draw, dstoch=gs.cuda() if use_s else None, dmean=gm.cuda() if use_m else None,
                       dstd=gd.cuda() if use_d else None, eps=eps.cuda() if use_s else None, mean_act=mean_act,
                       std_act=std_act, accumulate=accumulate)
    want = r64.grad + (base.double() if accumulate else 0.0)
    assert_grad_close(draw, want, what="draw")


@pytest.mark.parametrize("reset", ["none", "some", "all"])
@pytest.mark.parametrize("M,S", [(16, 8), (5, 30), (64, 64)])
def test_head_next_blend(ops, monkeypatch, M, S, reset):
    """next_out = stoch (1 - first) + init first: the reset blend of the next observe step (networks.py:183-191)."""
    raw, eps, _ = head_inputs(M, S, seed=3)
    g = torch.Generator().manual_seed(9)
    init = torch.randn(S, generator=g)
    first = {"none": torch.zeros(M), "all": torch.ones(M),
             "some": (torch.arange(M) % 3 == 1).float()}[reset]
    mean_r, std_r = ref_stats(raw.double(), S, "none", "sigmoid2", 0.1)
    stoch_r = ref_rsample(mean_r, std_r, eps.double(), monkeypatch)
    f = first.double()[:, None]
    next_r = stoch_r * (1.0 - f) + init.double()[None] * f
    stoch, nxt = torch.empty(M, S, device="cuda"), torch.full((M, S), float("nan"), device="cuda")
    ops.gauss_head_fwd(raw.cuda(), stoch, eps=eps.cuda(), mean_act="none", std_act="sigmoid2", min_std=0.1,
                       next_blend=(first.cuda(), init.cuda(), nxt))
    assert_close(stoch, stoch_r, what="stoch")
    assert_close(nxt, next_r, what="next_out")
    rows = first.bool()
    assert torch.equal(nxt.cpu()[~rows], stoch.cpu()[~rows])
    assert torch.equal(nxt.cpu()[rows], init[None].expand(M, S)[rows])


@pytest.mark.parametrize("M,S,skip", [(1, 30, 0), (16, 8, 0), (33, 7, 123), (1024, 32, 5), (15360, 64, 77), (3, 200, 1)])
def test_head_philox_eps_equals_fill_normal(ops, M, S, skip):
    """Without injected noise the head draws what dv3_fill_normal writes at the same stream position."""
    r1, r2 = ops.RngStream(torch.device("cuda"), seed=11), ops.RngStream(torch.device("cuda"), seed=11)
    for r in (r1, r2):
        r.take(skip)
    raw, _, _ = head_inputs(M, S, seed=4)
    want = ops.fill_normal(torch.empty(M, S, device="cuda"), r2)
    stoch, mean, std, eps_out = (torch.empty(M, S, device="cuda") for _ in range(4))
    ops.gauss_head_fwd(raw.cuda(), stoch, mean, std, rng=r1, eps_out=eps_out, mean_act="none", std_act="sigmoid2",
                       min_std=0.1)
    assert r1.cursor == r2.cursor
    assert torch.equal(eps_out, want)
    mean_r, std_r = ref_stats(raw.double(), S, "none", "sigmoid2", 0.1)
    assert_close(stoch, mean_r + std_r * want.cpu().double(), what="stoch")
    # the same draws once the device offset has moved (the position is state + launch argument)
    r1.commit(), r2.commit()
    want2 = ops.fill_normal(torch.empty(M, S, device="cuda"), r2)
    ops.gauss_head_fwd(raw.cuda(), stoch, rng=r1, eps_out=eps_out, mean_act="none", std_act="sigmoid2", min_std=0.1)
    assert torch.equal(eps_out, want2)
    assert not torch.equal(want, want2)


# ------------------------------------------------------------------------------------------------- KL
def ref_kl(pm, ps, qm, qs, free, dyn_scale, rep_scale):
    """RSSM.kl_loss of the reference (continuous branch) on float64 tensors -> (loss, value, ent_post, ent_prior)."""
    dist = lambda m, s: torchd.Independent(torchd.Normal(m, s), 1)
    kld = torchd.kl.kl_divergence
    rep = value = kld(dist(pm, ps), dist(qm.detach(), qs.detach()))
    dyn = kld(dist(pm.detach(), ps.detach()), dist(qm, qs))
    loss = dyn_scale * torch.clip(dyn, min=free) + rep_scale * torch.clip(rep, min=free)
    return loss, value, dist(pm, ps).entropy(), dist(qm, qs).entropy()


def kl_inputs(R, S, seed=0):
    g = torch.Generator().manual_seed(77 * S + R + seed)
    pm, qm = torch.randn(R, S, generator=g), torch.randn(R, S, generator=g)
    ps = 0.1 + 2.0 * torch.rand(R, S, generator=g)
    qs = 0.1 + 2.0 * torch.rand(R, S, generator=g)
    return pm, ps, qm, qs


def pick_free(value):
    """A free-bits floor that splits the rows: the midpoint of the widest gap between neighbouring KL values in the
    central half of their sorted order.  Every row must then lie further from the floor than fp32 rounding of a KL of
    that size (1e-5 of the floor is a hundred times that), so that the clip's mask is the same in fp32 and fp64 and
    the gradients of ALL rows are compared."""
    v = value.detach().flatten().sort().values
    n = v.numel()
    if n == 1:
        free = 1.0
    else:
        lo, hi = n // 4, max(n // 4 + 1, (3 * n) // 4)
        gaps = v[lo + 1:hi + 1] - v[lo:hi]
        i = int(gaps.argmax()) + lo
        free = float(0.5 * (v[i] + v[i + 1]))
        assert bool((v < free).any()) and bool((v > free).any())
    assert float((v - free).abs().min()) > 1e-5 * max(1.0, free), "no clean gap for the floor"
    return free


def run_kl(ops, pm, ps, qm, qs, free, dyn_scale, rep_scale, up):
    R, S = pm.shape
    d = [t.cuda() for t in (pm, ps, qm, qs)]
    kl, ep, eq = (torch.full((R,), float("nan"), device="cuda") for _ in range(3))
    ops.gauss_kl_fwd(*d, kl, ep, eq)
    outs = [torch.full((R, S), float("nan"), device="cuda") for _ in range(4)]
    ops.gauss_kl_bwd(*d, kl, dpost_mean=outs[0], dpost_std=outs[1], dprior_mean=outs[2], dprior_std=outs[3], free=free,
                     dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=up)
    return kl, ep, eq, outs


@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("R", M_LIST)
def test_kl_fwd_bwd(ops, R, S):
    pm, ps, qm, qs = kl_inputs(R, S)
    t64 = [t.double().requires_grad_(True) for t in (pm, ps, qm, qs)]
    dyn_scale, rep_scale, up = 0.5, 0.1, 1.0 / R
    with torch.no_grad():
        value0 = ref_kl(*t64, 0.0, dyn_scale, rep_scale)[1]
    free = pick_free(value0)  # the clip bites on part of the rows (on the only row or not when R == 1)
    loss, value, ent_p, ent_q = ref_kl(*t64, free, dyn_scale, rep_scale)
    (loss.sum() * up).backward()
    kl, ep, eq, outs = run_kl(ops, pm, ps, qm, qs, free, dyn_scale, rep_scale, up)
    assert_close(kl, value, what="kl")
    assert_close(ep, ent_p, what="ent_post")
    assert_close(eq, ent_q, what="ent_prior")
    for got, ref, nm in zip(outs, t64, ("dpost_mean", "dpost_std", "dprior_mean", "dprior_std")):
        assert_grad_close(got, ref.grad, what=nm)


@pytest.mark.parametrize("S", [1, 8, 30, 64, 200])
def test_kl_rows_at_below_and_above_free(ops, S):
    """unit std and a mean offset d give KL = S d^2 / 2 exactly, in fp32 and in fp64: d = 1, 2, 3 put a row below the
    floor free = 2 S, exactly on it and above it.  torch.clip passes the gradient at the floor (x >= min)."""
    d = torch.tensor([1.0, 2.0, 3.0, 2.0, 0.0])
    R = d.numel()
    pm, qm = d[:, None].expand(R, S).contiguous(), torch.zeros(R, S)
    ps, qs = torch.ones(R, S), torch.ones(R, S)
    free, dyn_scale, rep_scale, up = 2.0 * S, 0.5, 0.1, 0.25
    t64 = [t.double().requires_grad_(True) for t in (pm, ps, qm, qs)]
    loss, value, _, _ = ref_kl(*t64, free, dyn_scale, rep_scale)
    (loss.sum() * up).backward()
    kl, _, _, outs = run_kl(ops, pm, ps, qm, qs, free, dyn_scale, rep_scale, up)
    assert torch.equal(kl.cpu().double(), value.detach())
    assert kl.cpu().tolist() == [0.5 * S, 2.0 * S, 4.5 * S, 2.0 * S, 0.0]
    for got, ref, nm in zip(outs, t64, ("dpost_mean", "dpost_std", "dprior_mean", "dprior_std")):
        assert_grad_close(got, ref.grad, what=nm)
    assert bool((outs[0][0] == 0).all()) and bool((outs[0][4] == 0).all())      # below the floor: no gradient
    assert bool((outs[0][1] != 0).all()) and bool((outs[0][3] != 0).all())      # on the floor: passes
    assert bool((outs[2][2] != 0).all())                                        # above


@pytest.mark.parametrize("acc_post,acc_prior", [(False, False), (True, False), (False, True), (True, True)])
def test_kl_bwd_accumulate_and_null_outputs(ops, acc_post, acc_prior):
    R, S = 40, 30
    pm, ps, qm, qs = kl_inputs(R, S, seed=1)
    t64 = [t.double().requires_grad_(True) for t in (pm, ps, qm, qs)]
    dyn_scale, rep_scale, up = 0.5, 0.1, 1.0 / R
    with torch.no_grad():
        free = pick_free(ref_kl(*t64, 0.0, dyn_scale, rep_scale)[1])
    loss, value, _, _ = ref_kl(*t64, free, dyn_scale, rep_scale)
    (loss.sum() * up).backward()
    d = [t.cuda() for t in (pm, ps, qm, qs)]
    kl = torch.empty(R, device="cuda")
    ops.gauss_kl_fwd(*d, kl)  # entropies not requested
    base = [torch.randn(R, S, generator=torch.Generator().manual_seed(i)) for i in range(4)]
    outs = [b.cuda() for b in base]
    ops.gauss_kl_bwd(*d, kl, dpost_mean=outs[0], dpost_std=outs[1], dprior_mean=outs[2], dprior_std=outs[3], free=free,
                     dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=up, acc_post=acc_post, acc_prior=acc_prior)
    for i, (got, ref) in enumerate(zip(outs, t64)):
        acc = acc_post if i < 2 else acc_prior
        assert_grad_close(got, ref.grad + (base[i].double() if acc else 0.0), what=f"out{i}")
    # only the posterior's mean gradient wanted: the other three outputs stay untouched
    only = torch.full((R, S), float("nan"), device="cuda")
    ops.gauss_kl_bwd(*d, kl, dpost_mean=only, free=free, dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=up)
    assert_grad_close(only, t64[0].grad, what="dpost_mean only")


def test_wrappers_reject_bad_arguments_before_launching(ops):
    from dv3hip import _lib

    mk = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError):
        ops.gauss_head_fwd(mk(4, 15), mk(4, 7))                         # odd stat width
    with pytest.raises(ValueError):
        ops.gauss_head_fwd(mk(4, 16), mk(4, 7), eps=mk(4, 8))           # stoch width
    with pytest.raises(ValueError):
        ops.gauss_head_fwd(mk(4, 16), mk(4, 8))                         # sampling without eps or rng
    with pytest.raises(ValueError):
        ops.gauss_head_fwd(mk(4, 2 * 1025), mk(4, 1025), eps=mk(4, 1025))
    with pytest.raises(NotImplementedError):
        ops.gauss_head_fwd(mk(4, 16), mk(4, 8), eps=mk(4, 8), std_act="exp")
    with pytest.raises(TypeError):
        ops.gauss_head_fwd(torch.zeros(4, 16), mk(4, 8), eps=mk(4, 8))
    with pytest.raises(ValueError):
        ops.gauss_head_bwd(mk(4, 16), mk(4, 16), dstoch=mk(4, 8))       # sample backward without eps
    with pytest.raises(ValueError):
        ops.gauss_kl_fwd(mk(4, 8), mk(4, 8), mk(4, 8), mk(4, 7), mk(4))
    with pytest.raises(ValueError):
        ops.gauss_kl_bwd(mk(4, 8), mk(4, 8), mk(4, 8), mk(4, 8), mk(4), free=1.0, dyn_scale=0.5, rep_scale=0.1,
                         upstream=1.0)
    lib = _lib.load()
    assert lib.dv3_gauss_head_fwd(None, None, None, 0, None, None, None, None, 4, 8, 0, 0, 0.1, 0, None, None, None,
                                  None) == 10001
    assert lib.dv3_gauss_kl_fwd(None, None, None, None, None, None, None, 4, 8, None) == 10001
