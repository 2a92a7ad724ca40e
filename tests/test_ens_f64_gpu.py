"""Float64 parity of the member-batched ensemble kernels (csrc/ensops.hip), each ops.ens_* called directly (not through
dv3hip.engine.EnsembleEngine) at the edges of its host dispatch.

Every comparison is one kernel against a plain float64 PyTorch expression on the CPU (gradients: torch.autograd on that
expression); inputs are seeded fp32 tensors cast to float64; every reference takes `dt` so that
test_fp32_oracle_error_is_under_half_the_bar can evaluate it in fp32 on the CPU (never against a kernel).

  ens_gemm          three orientations x {stacked C, summed 2-D C} x {stacked A, shared 2-D A}; M, N in 1 .. 130 and K in
                    1 .. 67 around the 64 x 64 x 32 tile; 1, 2, 3, 10 members; bias (a summed C holds the SUM of the
                    members' biases); accumulate; padded row and member strides on a 4-byte-aligned base; a grid of 8
                    workgroups and grids that are no multiple of 8 (xcd_remap); EXACT on integers.
  ens_ln_act        forward and backward against float64 autograd at both edges of all six register depths (N = 1 ..
                    2048), rows that straddle two members, the second trip of the backward's row loop (M = 257),
                    gamma with a member stride > N, dgamma None / prefilled, an odd ldx, act codes 0, 1 and a runtime
                    code, the LayerNorm row kinds of tests/test_ln_gru_f64_gpu.py.
  ens_colsum        M = 1 .. 5, 130 x N = 1 .. 200, accumulate, strides; EXACT on integers.
  ens_regress_loss  K M W = 200, 262144 (the 1024-workgroup cap) and 262145 (its first grid-stride trip); a strided
                    target; dpre aliasing pre; saturated pre; the ticket reset (two calls, one workspace, equal bits).
  ens_disag_*       M, W, U around the tile, 2 / 3 / 10 members, mu None / given (bit-equal reward), log / scale,
                    reward and dreward as a column of a wider buffer; identical members pin the convention disag = 0,
                    reward = -inf (log) or 0, backward all zeros (torch.std's gradient there is NaN).

Bars: values 1e-4 * max(1, max |ref|) (TOL of tests/test_kernels_gpu.py); gradients GTOL = 3e-4 of the tensor's own
maximum (tests/test_ens_kernels_gpu.py).  The disagreement cases assert, in the reference, that the smallest std over
members is >= 1e-3 max |mu|: a condition on the inputs, not a tolerance.  No bar is widened.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.test_ln_gru_f64_gpu import rows_of
from tests.test_row_kernels_f64_gpu import check, dev, gen

TOL = 1e-4
GTOL = 3e-4
EPS = 1e-3
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
PAD = 7777.0
ERR_ARG = 10001
RT_ACT = "Tanh"
LN_KINDS = ["randn", "offset", "tiny", "spike", "const"]
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def seed_of(c, salt=0):
    return zlib.crc32(repr(sorted(c.items())).encode()) % 1000003 + salt


def ints(shape, g):
    return torch.randint(-3, 4, tuple(shape), generator=g).float()


def exact(got, ref, what):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int((got != ref).sum())
    print(f"{what}: exact" if bad == 0 else f"{what}: {bad} of {ref.numel()} differ")
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"


def ratio(r32, r64, tol=TOL, floor=1.0):
    r64 = r64.double()
    err, bar = (r32.double() - r64).abs().max().item(), tol * max(floor, r64.abs().max().item())
    return 0.0 if err == 0.0 else err / bar if bar else math.inf


def strided(t, row_pad=0, mem_pad=0, off=0, v=PAD):
    """A GPU copy of t ([R, C] or [K, R, C]) as a view of a larger buffer of v: row stride C + row_pad, member stride
    R * ld + mem_pad, first element `off` floats into the buffer (off = 1: a 4-byte-aligned base)."""
    if t.dim() == 2:
        return strided(t[None], row_pad, mem_pad, off, v)[0]
    K, R, C = t.shape
    ld = C + row_pad
    st = R * ld + mem_pad
    buf = torch.full((off + K * st + 8,), v, device="cuda")
    view = buf.as_strided((K, R, C), (st, ld, 1), off)
    view.copy_(t)
    return view


def act_fn(z, act):
    if act in (False, 0):
        return z
    if act in (True, 1):
        return F.silu(z)
    assert act == RT_ACT
    return torch.tanh(z)


# ============================================================================================================ ens_gemm
ORIENT = {"NT": (False, True), "NN": (False, False), "TN": (True, False)}
# (M, N, K, members)
EG_SHAPES = [(1, 63, 1, 1), (1, 130, 31, 2), (63, 1, 32, 3), (64, 64, 33, 10), (65, 65, 67, 2), (130, 63, 32, 3),
             (128, 128, 32, 2), (64, 64, 32, 8)]


def EG(o, M, N, K, Kb, summed, shared, bias=True, acc=False, pad=False):
    return dict(o=o, M=M, N=N, K=K, Kb=Kb, summed=summed, shared=shared, bias=bias, acc=acc, pad=pad)


EG_CASES = [EG(o, M, N, K, Kb, summed, shared, bias=(i + j) % 2 == 0, acc=(i + j) % 3 == 0, pad=(i + j) % 2 == 1)
            for j, o in enumerate(ORIENT) for summed in (False, True) for shared in (False, True)
            for i, (M, N, K, Kb) in enumerate(EG_SHAPES)]


def eg_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def eg_grid(c):
    """Workgroups of the launch (csrc/ensops.hip dv3_ens_gemm_f32)."""
    return -(-c["M"] // 64) * -(-c["N"] // 64) * (1 if c["summed"] else c["Kb"])


def eg_inputs(c, kind):
    ta, tb = ORIENT[c["o"]]
    M, N, K, Kb = c["M"], c["N"], c["K"], c["Kb"]
    g = gen(seed_of(c, 977 if kind == "int" else 0))
    draw = (lambda *s: ints(s, g)) if kind == "int" else (lambda *s: torch.randn(*s, generator=g))
    A = draw(*((K, M) if ta else (M, K))) if c["shared"] else draw(Kb, *((K, M) if ta else (M, K)))
    B = draw(Kb, *((N, K) if tb else (K, N)))
    if kind != "int":
        B = B / math.sqrt(K)
    bias = draw(Kb, N) if c["bias"] else None
    C0 = draw(M, N) if c["summed"] else draw(Kb, M, N)
    return A, B, bias, C0


def eg_ref(c, A, B, bias, C0, dt=F64):
    ta, tb = ORIENT[c["o"]]
    A3 = (A[None].expand(c["Kb"], -1, -1) if A.dim() == 2 else A).to(dt)
    C = (A3.transpose(1, 2) if ta else A3) @ (B.to(dt).transpose(1, 2) if tb else B.to(dt))
    if bias is not None:
        C = C + bias.to(dt)[:, None, :]
    if c["summed"]:
        C = C.sum(0)
    return C + C0.to(dt) if c["acc"] else C


@gpu
@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("c", EG_CASES, ids=eg_id)
def test_ens_gemm(ops, c, kind):
    ta, tb = ORIENT[c["o"]]
    A, B, bias, C0 = eg_inputs(c, kind)
    ref = eg_ref(c, A, B, bias, C0)
    rp, mp, off = (3, 5, 1) if c["pad"] else (0, 0, 0)
    Ad, Bd = strided(A, rp, mp, off), strided(B, rp, mp, off)
    Cd = strided(C0 if c["acc"] else torch.full(C0.shape, NAN), rp, mp, off, NAN)
    bd = None if bias is None else strided(bias[None], rp, 0, off)[0]
    assert not c["pad"] or Ad.data_ptr() % 16 == 4
    ops.ens_gemm(Ad, Bd, Cd, bias=bd, transA=ta, transB=tb, accumulate=c["acc"])
    what = f"ens_gemm {eg_id(c)} grid {eg_grid(c)} {kind}"
    if kind == "int":
        assert c["Kb"] * (9 * c["K"] + 3) + 3 < 2 ** 23  # every partial sum is an integer fp32 holds
        exact(Cd, ref, what)
    else:
        check(Cd, ref, what=what)


def test_ens_gemm_grids_cover_the_xcd_remap():
    grids = {eg_grid(c) for c in EG_CASES}
    assert any(g % 8 == 0 for g in grids) and any(g % 8 and g > 8 for g in grids), sorted(grids)


# ========================================================================================================== ens_ln_act
ELN_N = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
ELN_KM = [(1, 1), (2, 3), (3, 5), (2, 257)]  # (members, rows): 3 and 5 rows: a workgroup's four rows straddle members


def ELN(K, M, N, act=True, kind="randn", gstride=0, ldpad=0, dgamma="fill"):
    return dict(K=K, M=M, N=N, act=act, kind=kind, gstride=gstride, ldpad=ldpad, dgamma=dgamma)


ELN_CASES = ([ELN(*ELN_KM[i % 4], N) for i, N in enumerate(ELN_N)] +
             [ELN(2, 257, N) for N in (64, 129, 1025)] + [ELN(3, 5, N) for N in (64, 513, 2048)] +
             [ELN(3, 5, 65, gstride=7), ELN(3, 5, 65, dgamma=None), ELN(3, 5, 66, ldpad=3), ELN(2, 3, 130, ldpad=1, gstride=2),
              ELN(3, 5, 65, act=False), ELN(3, 5, 65, act=RT_ACT), ELN(2, 3, 300, act=RT_ACT), ELN(2, 257, 1100, act=False)] +
             [ELN(3, 5, 65, kind=k) for k in LN_KINDS[1:]])


def eln_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def eln_inputs(c):
    K, M, N = c["K"], c["M"], c["N"]
    g = gen(seed_of(c, 3))
    x = rows_of(K * M, N, c["kind"], g).reshape(K, M, N)
    gamma, beta = 1 + 0.1 * torch.randn(K, N, generator=g), 0.1 * torch.randn(K, N, generator=g)
    dy = torch.randn(K, M, N, generator=g)
    dg0, db0 = torch.randn(K, N, generator=g), torch.randn(K, N, generator=g)
    return x, gamma, beta, dy, dg0, db0


def eln_ref(c, x, gamma, beta, dy, dt=F64):
    xr, gr, br = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (x, gamma, beta))
    mean = xr.mean(-1, keepdim=True)
    d = xr - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS)
    y = act_fn(d * rstd * gr[:, None, :] + br[:, None, :], c["act"])
    y.backward(dy.to(dt))
    return dict(y=y.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), dx=xr.grad, dgamma=gr.grad,
                dbeta=br.grad)


def eln_floor(c, k):
    """rstd of the spiked rows and every gradient are held to their own maximum; dgamma / dbeta include the prefill."""
    return 0.0 if (k == "rstd" and c["kind"] == "spike") or k == "dx" else 1.0


ELN_TOL = dict(y=TOL, mean=TOL, rstd=TOL, dx=GTOL, dgamma=GTOL, dbeta=GTOL)


def eln_ratio(c):
    x, gamma, beta, dy, dg0, db0 = eln_inputs(c)
    a, b = eln_ref(c, x, gamma, beta, dy, F32), eln_ref(c, x, gamma, beta, dy, F64)
    return max(ratio(a[k], b[k], ELN_TOL[k], eln_floor(c, k)) for k in b)


@gpu
@pytest.mark.parametrize("c", ELN_CASES, ids=eln_id)
def test_ens_ln_act(ops, c):
    K, M, N = c["K"], c["M"], c["N"]
    x, gamma, beta, dy, dg0, db0 = eln_inputs(c)
    ref = eln_ref(c, x, gamma, beta, dy)
    what = "ens_ln_act " + eln_id(c)
    rows = lambda t, v=PAD: strided(t, c["ldpad"], 0, 0, v)  # the members' rows back to back
    vec = lambda t: strided(t[None], c["gstride"], 0, 0)[0]
    xd, gd, bd = rows(x), vec(gamma), vec(beta)
    y = rows(torch.full((K, M, N), NAN), NAN)
    mean, rstd = torch.full((K * M,), NAN, device="cuda"), torch.full((K * M,), NAN, device="cuda")
    ops.ens_ln_act_fwd(xd, gd, bd, y, mean, rstd, act=c["act"])
    for k, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        check(got, ref[k], what=f"{what} {k}", floor=eln_floor(c, k))
    dx = rows(torch.full((K, M, N), NAN), NAN)
    dg, db = (vec(dg0), vec(db0)) if c["dgamma"] else (None, None)
    ops.ens_ln_act_bwd(rows(dy), xd, gd, bd, mean, rstd, dx, dg, db, act=c["act"])
    check(dx, ref["dx"], tol=GTOL, what=what + " dx", floor=0.0)
    if c["dgamma"]:
        check(dg, ref["dgamma"] + dg0.double(), tol=GTOL, what=what + " dgamma")
        check(db, ref["dbeta"] + db0.double(), tol=GTOL, what=what + " dbeta")


@gpu
def test_ens_ln_act_rejects_2049_columns():
    from dv3hip import _lib

    K, M, N = 2, 3, 2049
    x, v = dev(torch.randn(K * M, N)), dev(torch.ones(K, N))
    y, dx = torch.full((K * M, N), NAN, device="cuda"), torch.full((K * M, N), NAN, device="cuda")
    mean, rstd = torch.full((K * M,), NAN, device="cuda"), torch.full((K * M,), NAN, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    assert lib.dv3_ens_ln_act_fwd(x.data_ptr(), N, v.data_ptr(), v.data_ptr(), N, y.data_ptr(), N, mean.data_ptr(),
                                  rstd.data_ptr(), K, M, N, s) == ERR_ARG
    assert lib.dv3_ens_ln_act_bwd(x.data_ptr(), N, x.data_ptr(), N, v.data_ptr(), v.data_ptr(), N, mean.data_ptr(),
                                  rstd.data_ptr(), dx.data_ptr(), N, 0, 0, K, M, N, s) == ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, dx, mean, rstd)), "an output was written"


# ========================================================================================================== ens_colsum
ECS_CASES = [(K, M, N, pad) for i, (K, M) in enumerate(((1, 1), (2, 2), (3, 3), (2, 4), (10, 5), (3, 130)))
             for j, N in enumerate((1, 63, 64, 65, 200)) for pad in [(i + j) % 2 == 1]]


def ecs_inputs(K, M, N, kind):
    g = gen(K * 1009 + M * 31 + N + (977 if kind == "int" else 0))
    draw = (lambda *s: ints(s, g)) if kind == "int" else (lambda *s: torch.randn(*s, generator=g))
    return draw(K, M, N), draw(K, N)


def ecs_ref(x, out0, acc, dt=F64):
    s = x.to(dt).sum(1)
    return s + out0.to(dt) if acc else s


@gpu
@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("K,M,N,pad", ECS_CASES)
def test_ens_colsum(ops, K, M, N, pad, kind):
    x, out0 = ecs_inputs(K, M, N, kind)
    xd = strided(x, 3, 5, 1) if pad else dev(x)
    for acc in (False, True):
        out = strided((out0 if acc else torch.full((K, N), NAN))[None], 2 if pad else 0, 0, 0, NAN)[0]
        ops.ens_colsum(xd, out, accumulate=acc)
        what = f"ens_colsum {K}x{M}x{N} pad={pad} acc={acc} {kind}"
        if kind == "int":
            assert 3 * (M + 1) < 2 ** 23
            exact(out, ecs_ref(x, out0, acc), what)
        else:
            check(out, ecs_ref(x, out0, acc), what=what)


# ==================================================================================================== ens_regress_loss
ERL_CASES = [(2, 10, 10), (2, 512, 256), (5, 109, 481)]  # K M W = 200, 262144 (1024 workgroups), 262145 (the first stride)
ERL_STD = 0.7


def erl_inputs(K, M, W):
    g = gen(K * M * W % 99991)
    pre = torch.randn(K, M, W, generator=g)
    pre.view(-1)[::97] = 20.0
    pre.view(-1)[5::101] = -20.0
    return pre, torch.tanh(torch.randn(M, W, generator=g))


def erl_ref(pre, target, dt=F64):
    p = pre.detach().to(dt, copy=True).requires_grad_(True)
    mu = torch.tanh(p)
    logp = -0.5 * ((target.to(dt)[None] - mu) / ERL_STD) ** 2 - math.log(ERL_STD) - 0.5 * math.log(2 * math.pi)
    loss = -logp.sum(-1).mean()
    loss.backward()
    return loss.detach().reshape(1), p.grad


@gpu
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("K,M,W", ERL_CASES)
def test_ens_regress_loss(ops, K, M, W, alias):
    assert K * M * W in (200, 262144, 262145)
    pre, target = erl_inputs(K, M, W)
    loss_ref, dpre_ref = erl_ref(pre, target)
    pd, td = dev(pre), strided(target, 3, 0, 1)
    dpre = pd if alias else torch.full((K, M, W), NAN, device="cuda")
    ws, loss = torch.zeros(ops.ENS_LOSS_WS, device="cuda"), torch.full((1,), NAN, device="cuda")
    ops.ens_regress_loss(pd, td, dpre, loss, ws, ERL_STD)
    what = f"ens_regress_loss {K}x{M}x{W} alias={alias}"
    check(loss, loss_ref, what=what + " loss")
    check(dpre, dpre_ref, tol=GTOL, what=what + " dpre", floor=0.0)
    first = loss.clone()
    loss.fill_(NAN)
    ops.ens_regress_loss(dev(pre), td, torch.empty(K, M, W, device="cuda"), loss, ws, ERL_STD)  # same workspace: the ticket was reset
    assert torch.equal(loss.cpu(), first.cpu()), (what, "the second call on the same workspace gave another loss")


# ========================================================================================================= ens_disag_*
def ED(K, M, W, U, log=True, scale=1.0):
    return dict(K=K, M=M, W=W, U=U, log=log, scale=scale)


ED_CASES = [ED(2, 1, 1, 1), ED(3, 63, 31, 31, log=False, scale=0.7), ED(10, 65, 33, 33, scale=0.7), ED(2, 257, 64, 67),
            ED(3, 63, 65, 31, log=False), ED(10, 65, 130, 33)]


def ed_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def ed_inputs(c):
    """Members = a common part + a tenth of it in member noise, biases 0.4 apart: the members' predictions differ by
    design (the condition below) while the head product still carries the values."""
    K, M, W, U = c["K"], c["M"], c["W"], c["U"]
    g = gen(seed_of(c, 4))
    h = torch.randn(1, M, U, generator=g) + 0.1 * torch.randn(K, M, U, generator=g)
    w = 0.5 * (torch.randn(1, W, U, generator=g) + 0.1 * torch.randn(K, W, U, generator=g)) / math.sqrt(U)
    bias = 0.4 * (torch.arange(K).float()[:, None] - (K - 1) / 2) + 0.05 * torch.randn(K, W, generator=g)
    return h, w, bias, torch.randn(M, generator=g)


def ed_ref(c, h, w, bias, drew, dt=F64):
    pre = (h.to(dt) @ w.to(dt).transpose(1, 2) + bias.to(dt)[:, None, :]).requires_grad_(True)
    mu = torch.tanh(pre)
    disag = mu.std(0).mean(-1)
    reward = c["scale"] * (torch.log(disag) if c["log"] else disag)
    (dpre,) = torch.autograd.grad((reward * drew.to(dt)).sum(), pre)
    return dict(mu=mu.detach(), disag=disag.detach(), reward=reward.detach(), dpre=dpre)


def ed_ratio(c):
    t = ed_inputs(c)
    a, b = ed_ref(c, *t, dt=F32), ed_ref(c, *t, dt=F64)
    assert b["mu"].std(0).min().item() >= 1e-3 * b["mu"].abs().max().item(), c  # a condition on the inputs
    return max(ratio(a[k], b[k], GTOL if k == "dpre" else TOL, 0.0 if k == "dpre" else 1.0) for k in b)


def ed_fwd(ops, c, h, w, bias, with_mu, column):
    K, M, W = c["K"], c["M"], c["W"]
    hd, wd, bd = strided(h, 3, 5, 1), strided(w, 1, 2, 0), strided(bias[None], 2, 0, 0)[0]
    rbuf = torch.full((M, 3), NAN, device="cuda")
    reward = rbuf[:, 1:2] if column else torch.full((M,), NAN, device="cuda")
    disag, part = torch.full((M,), NAN, device="cuda"), torch.full((-(-W // 64) * M,), NAN, device="cuda")
    mu = torch.full((K, M, W), NAN, device="cuda") if with_mu else None
    ops.ens_disag_fwd(hd, wd, bd, reward, disag, part, mu=mu, scale=c["scale"], log=c["log"])
    if column:
        assert bool(torch.isnan(rbuf[:, 0]).all()) and bool(torch.isnan(rbuf[:, 2]).all()), "wrote outside the reward column"
    return reward.reshape(M), disag, mu


@gpu
@pytest.mark.parametrize("c", ED_CASES, ids=ed_id)
def test_ens_disag(ops, c):
    K, M, W = c["K"], c["M"], c["W"]
    h, w, bias, drew = ed_inputs(c)
    ref = ed_ref(c, h, w, bias, drew)
    assert ref["mu"].std(0).min().item() >= 1e-3 * ref["mu"].abs().max().item()
    what = "ens_disag " + ed_id(c)
    r0, d0, _ = ed_fwd(ops, c, h, w, bias, False, False)
    reward, disag, mu = ed_fwd(ops, c, h, w, bias, True, True)
    assert torch.equal(r0.cpu(), reward.cpu()) and torch.equal(d0.cpu(), disag.cpu()), what + ": mu changes the reward"
    check(reward, ref["reward"], what=what + " reward")
    check(disag, ref["disag"], what=what + " disag")
    check(mu, ref["mu"], what=what + " mu")
    dbuf = torch.full((M, 3), PAD, device="cuda")
    dbuf[:, 2] = dev(drew)
    ops.ens_disag_bwd(mu, disag, dbuf[:, 2:3], scale=c["scale"], log=c["log"])
    check(mu, ref["dpre"], tol=GTOL, what=what + " dpre", floor=0.0)


@gpu
@pytest.mark.parametrize("log", [True, False])
def test_ens_disag_identical_members(ops, log):
    """All members equal: disag is exactly 0, the reward -inf (log) or 0, and the backward all zeros -- the kernels'
    convention where torch.std's gradient is NaN."""
    c = ED(3, 65, 33, 31, log=log, scale=0.7)
    h, w, bias, drew = ed_inputs(c)
    h, w, bias = (t[:1].expand(3, -1, -1).contiguous() for t in (h, w, bias[:, None, :]))
    reward, disag, mu = ed_fwd(ops, c, h, w, bias[:, 0, :], True, False)
    assert bool((disag == 0).all()), "disag of identical members is not exactly 0"
    assert bool((reward == (-math.inf if log else 0.0)).all()), reward[:4]
    ops.ens_disag_bwd(mu, disag, dev(drew), scale=0.7, log=log)
    assert bool((mu == 0).all()), "the backward of identical members is not all zeros"


# ============================================================================================ the oracle's own error
def group_ratios():
    worst = {"gemm": 0.0, "colsum": 0.0, "loss": 0.0}
    for c in EG_CASES:
        A, B, bias, C0 = eg_inputs(c, "randn")
        worst["gemm"] = max(worst["gemm"], ratio(eg_ref(c, A, B, bias, C0, F32), eg_ref(c, A, B, bias, C0)))
    for K, M, N, _ in ECS_CASES:
        x, o = ecs_inputs(K, M, N, "randn")
        worst["colsum"] = max(worst["colsum"], ratio(ecs_ref(x, o, True, F32), ecs_ref(x, o, True)))
    for K, M, W in ERL_CASES:
        pre, target = erl_inputs(K, M, W)
        (l32, g32), (l64, g64) = erl_ref(pre, target, F32), erl_ref(pre, target)
        worst["loss"] = max(worst["loss"], ratio(l32, l64), ratio(g32, g64, GTOL, 0.0))
    worst["ln"] = max(eln_ratio(c) for c in ELN_CASES)
    worst["disag"] = max(ed_ratio(c) for c in ED_CASES)
    return worst


def test_fp32_oracle_error_is_under_half_the_bar():
    """No bar is widened: on every case the same reference evaluated in fp32 on the CPU stays under half of the bar
    from the float64 one; the disagreement inputs meet their condition.  CPU only; no kernel is involved."""
    worst = group_ratios()
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v < 0.5 for v in worst.values()), worst
