"""Layer activation codes 0..6 (include/dv3hip.h: none, SiLU, ReLU, ELU, GELU, Tanh, Mish) in every kernel that applies
the activation behind a LayerNorm, forward and backward, against float64 torch on the host (F.relu / elu / gelu / tanh /
mish + layer_norm + autograd).  The comparison rule is tests/test_row_kernels_f64_gpu.py's `check`, imported:
max |got - ref| <= 1e-4 * max(1, max |ref|), and no non-finite output.

Every fused site takes the code, so each is also compared with the unfused pair at the same code
to the equality its existing SiLU test asserts (tests/test_kernels_gpu.py, tests/test_ens_kernels_gpu.py).  The one
SiLU-only site, the LayerNorm-on-load prologue of dv3_gemm_sample_f32, is not launched by the engine for any layer:
RSSMEngine.img_step_fwd runs ln_act_fwd with the layer's code first (asserted below from the launch record).

Inputs: LayerNorm scale 1 + 0.1 randn, shift 0.1 randn; the `wide` case of every code sets two shifts to +46 and -46,
so that pre-activations reach beyond +-40 (asserted; finite values and gradients are part of `check`).  For ReLU the inputs are nudged
until no pre-activation lies within 1e-3 of zero (the derivative's jump)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_ens_kernels_gpu import GTOL
from tests.test_ens_kernels_gpu import close as ens_close
from tests.test_kernels_gpu import TOL, assert_close
from tests.test_row_kernels_f64_gpu import check, dev, gen

pytestmark = pytest.mark.gpu

F64 = torch.float64
CODES = [0, 1, 2, 3, 4, 5, 6]
NAMES = {0: "none", 1: "SiLU", 2: "ReLU", 3: "ELU", 4: "GELU", 5: "Tanh", 6: "Mish"}
EPS = 1e-3  # every LayerNorm on the path


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def act64(z, code):
    return {0: lambda t: t, 1: F.silu, 2: F.relu, 3: F.elu, 4: F.gelu, 5: torch.tanh, 6: F.mish}[code](z)


def ln_act64(x, gamma, beta, code):
    """act(LayerNorm(x) * gamma + beta) in float64; gamma / beta [N] or, per row block, broadcastable."""
    x = x.to(F64)
    xh = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    return act64(xh * gamma.to(F64) + beta.to(F64), code)


def make_ln_inputs(R, N, code, wide, seed, x_scale=1.5):
    """x [R,N], gamma, beta [N], dy [R,N] (fp32).  wide: shifts of +40 / -40 on two columns.  ReLU: no pre-activation
    within 1e-3 of zero."""
    g = gen(seed)
    x = torch.randn(R, N, generator=g) * x_scale + 0.2
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    if wide:
        beta[0], beta[N // 2] = 46.0, -46.0  # (|xhat gamma| stays below 6: these columns lie beyond +-40 on every row)
    dy = torch.randn(R, N, generator=g)
    if code == 2:
        for _ in range(50):
            z = ln_act64(x, gamma, beta, 0)
            bad = z.abs() < 1e-3
            if not bad.any():
                break
            x = x + 0.05 * bad.float()
        assert not bad.any()
    if wide:
        z = ln_act64(x, gamma, beta, 0)
        assert z.max() >= 40.0 and z.min() <= -40.0
    return x, gamma, beta, dy


def ref_fwd_bwd(x, gamma, beta, dy, code, params=True):
    xr = x.to(F64).requires_grad_(True)
    gr, br = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    y = ln_act64(xr, gr, br, code)
    y.backward(dy.to(F64))
    mean = x.to(F64).mean(-1)
    rstd = 1.0 / torch.sqrt(x.to(F64).var(-1, unbiased=False) + EPS)
    return y.detach(), mean, rstd, xr.grad, gr.grad, br.grad


def ln_bwd_ws(ops, dy, x, gamma, beta, mean, rstd, dx, dgamma, dbeta, code):
    """dv3_ln_act_bwd_ws (the two-stage parameter-gradient form ops.ln_act_bwd takes above 2 M elements) at any size."""
    R, N = x.shape
    ws = ops._ln_partials(x.device)
    ops._call("dv3_ln_act_bwd_ws", dy.data_ptr(), N, x.data_ptr(), N, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), dx.data_ptr(), N, dgamma.data_ptr(), dbeta.data_ptr(), R, N, code, 0, 0, ws.data_ptr(),
              ws.numel(), ops._stream())


# generic path (6, 130: not a multiple of 4 / below 16), vector path at 4 lanes (16) and 32 lanes (96) per row, and
# 2, 4 and 8 float4 chunks per lane (512, 1024, 2048)
@pytest.mark.parametrize("N", [6, 16, 96, 130, 512, 1024, 2048])
@pytest.mark.parametrize("R", [5, 300])
@pytest.mark.parametrize("code", CODES)
def test_ln_act_fwd_bwd_every_code(ops, code, R, N):
    for wide in (False, True):
        if wide and not (R == 300 or N == 6):  # (the +-40 case once per code and path is enough for R = 5)
            continue
        x, gamma, beta, dy = make_ln_inputs(R, N, code, wide, 100 * code + R + N + int(wide))
        y_ref, mean_ref, rstd_ref, dx_ref, dg_ref, db_ref = ref_fwd_bwd(x, gamma, beta, dy, code)
        what = f"{NAMES[code]} R={R} N={N} wide={wide}"
        xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
        y, mean, rstd = dev(torch.full((R, N), 7.0)), dev(torch.full((R,), 7.0)), dev(torch.full((R,), 7.0))
        ops.ln_act_fwd(xd, gd, bd, y, mean, rstd, act=code)
        check(y, y_ref, what=what + " y")
        check(mean, mean_ref, what=what + " mean")
        check(rstd, rstd_ref, what=what + " rstd")
        variants = [("bwd", True), ("bwd no params", False)]
        if N <= 512:
            variants.append(("bwd_ws", True))
        for tag, params in variants:
            dx = dev(torch.full((R, N), 7.0))
            dg, db = dev(torch.ones(N)), dev(torch.ones(N))  # (accumulated into)
            if tag == "bwd_ws":
                ln_bwd_ws(ops, dyd, xd, gd, bd, mean, rstd, dx, dg, db, code)
            else:
                ops.ln_act_bwd(dyd, xd, gd, bd, mean, rstd, dx, dg if params else None, db if params else None, act=code)
            check(dx, dx_ref, what=f"{what} {tag} dx")
            if params:
                check(dg - 1, dg_ref, what=f"{what} {tag} dgamma")
                check(db - 1, db_ref, what=f"{what} {tag} dbeta")


@pytest.mark.parametrize("code", CODES)
def test_ln_act_chw_group_every_code(ops, code):
    """The (C,H,W)-flatten addressing of the encoder's last layer: N = 8 channels, G = 16 pixels per image."""
    N, G, imgs = 8, 16, 3
    R = imgs * G
    x, gamma, beta, dy = make_ln_inputs(R, N, code, True, 900 + code)
    y_ref, _, _, dx_ref, dg_ref, db_ref = ref_fwd_bwd(x, gamma, beta, dy, code)
    chw = lambda t: t.reshape(imgs, G, N).permute(0, 2, 1).reshape(imgs, N * G).contiguous()
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    y, mean, rstd = dev(torch.full((imgs, N * G), 7.0)), dev(torch.empty(R)), dev(torch.empty(R))
    ops.ln_act_fwd(xd, gd, bd, y, mean, rstd, act=code, chw_group=G)
    check(y, chw(y_ref), what=f"{NAMES[code]} chw y")
    dx, dg, db = dev(torch.full((R, N), 7.0)), dev(torch.zeros(N)), dev(torch.zeros(N))
    ops.ln_act_bwd(dev(chw(dy)), xd, gd, bd, mean, rstd, dx, dg, db, act=code, chw_group=G)
    check(dx, dx_ref, what=f"{NAMES[code]} chw dx")
    check(dg, dg_ref, what=f"{NAMES[code]} chw dgamma")
    check(db, db_ref, what=f"{NAMES[code]} chw dbeta")


def test_unknown_code_is_rejected_before_any_launch(ops):
    from dv3hip import _lib

    x, g, b = dev(torch.randn(4, 16)), dev(torch.ones(16)), dev(torch.zeros(16))
    y = dev(torch.full((4, 16), 7.0))
    with pytest.raises(NotImplementedError):
        ops.ln_act_fwd(x, g, b, y, act=7)
    with pytest.raises(NotImplementedError):
        ops.act_code("Softsign")
    lib = _lib.load()
    for code in (7, -1):
        assert lib.dv3_ln_act_fwd(x.data_ptr(), 16, g.data_ptr(), b.data_ptr(), y.data_ptr(), 16, 0, 0, 4, 16, code, 0,
                                  ops._stream()) == 10001
        assert lib.dv3_ens_ln_act_fwd_ex(x.data_ptr(), 16, g.data_ptr(), b.data_ptr(), 0, y.data_ptr(), 16, x.data_ptr(),
                                         x.data_ptr(), 1, 4, 16, code, ops._stream()) == 10001
        assert lib.dv3_scan_ln_factors_ex(x.data_ptr(), 16, g.data_ptr(), b.data_ptr(), x.data_ptr(), x.data_ptr(),
                                          y.data_ptr(), y.data_ptr(), 4, 16, code, ops._stream()) == 10001
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 == float(y.max())


# ------------------------------------------------------------------------------------------ the fused sites
@pytest.mark.parametrize("M,N,S,D,A2", [(7, 16, 4, 4, 3), (5, 256, 8, 8, 2)])  # the generic and the vector kernel
@pytest.mark.parametrize("code", CODES)
def test_onehot_linear_ln_every_code(ops, code, M, N, S, D, A2):
    g = gen(31 * M + N + code)
    K = S * D + A2
    W = torch.randn(N, K, generator=g) / math.sqrt(S + A2 + 1)
    idx = torch.randint(0, D, (M, S), generator=g, dtype=torch.int32)
    x2 = torch.randn(M, A2, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    beta[1], beta[2] = 40.0, -40.0
    for _ in range(50):
        xfull = torch.cat([F.one_hot(idx.long(), D).float().reshape(M, S * D), x2], -1)
        pre_ref = xfull.to(F64) @ W.to(F64).t()
        bad = (ln_act64(pre_ref, gamma, beta, 0).abs() < 1e-3).any(-1)
        if code != 2 or not bad.any():
            break
        x2 = x2 + 0.05 * bad.float()[:, None] * torch.randn(M, A2, generator=g)  # (ReLU: away from the jump)
    assert code != 2 or not bad.any()
    y_ref = ln_act64(pre_ref, gamma, beta, code)
    WT = torch.empty(K, N, device="cuda")
    ops.transpose2d(dev(W), WT)
    mk = lambda *s: torch.full(s, 7.0, device="cuda")
    pre, y, mean, rstd = mk(M, N), mk(M, N), mk(M), mk(M)
    ops.onehot_linear_ln(dev(idx), D, WT, pre, x2=dev(x2), gamma=dev(gamma), beta=dev(beta), y=y, mean=mean, rstd=rstd,
                         act=code)
    check(pre, pre_ref, what="pre")
    check(y, y_ref, what=f"{NAMES[code]} gather y vs float64")
    # the unfused pair at the same code: dense Linear on the one-hot expansion, then ln_act_fwd
    pre_u, y_u, m_u, r_u = mk(M, N), mk(M, N), mk(M), mk(M)
    ops.gemm(dev(xfull), dev(W), pre_u)
    ops.ln_act_fwd(pre_u, dev(gamma), dev(beta), y_u, m_u, r_u, act=code)
    assert_close(y, y_u.cpu(), what=f"{NAMES[code]} gather y vs gemm + ln_act_fwd")
    assert_close(mean, m_u.cpu(), what="mean"), assert_close(rstd, r_u.cpu(), what="rstd")


def test_sample_plus_img_in_launch_is_bypassed_for_other_activations(ops):
    """dv3_onehot_sample_linear_ln_fwd keeps codes 0 and 1 (its 1024-thread form has no registers for the runtime
    switch): the entry rejects any other code before a launch, and the observe scan of an ELU model launches the sampler
    and the gather with the code instead (at a shape where a SiLU model takes the fused launch)."""
    import networks
    from dv3hip import _lib

    assert ops.sample_linear_ln_ok(4, 32, 256) and ops.sample_linear_ln_ok(4, 32, 256, False)
    assert not any(ops.sample_linear_ln_ok(4, 32, 256, c) for c in (2, 3, 4, 5, 6))
    M, S, D, N = 2, 4, 32, 256
    mk = lambda *sh: torch.zeros(*sh, device="cuda")
    mki = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.onehot_sample_linear_ln(mk(M, S, D), mk(M, S, D), next_first=mk(M), init=mk(S * D), init_idx=mki(S),
                                    next_out=mk(M, S, D), next_idx=mki(M * S), WT=mk(S * D, N), x2=None, pre=mk(M, N),
                                    gamma=mk(N), beta=mk(N), y=mk(M, N), mean=mk(M), rstd=mk(M), noise=mk(M, S, D) + 1,
                                    act="ELU")
    keys = {}
    for act in ("SiLU", "ELU"):
        torch.manual_seed(0)
        dyn = networks.RSSM(4, 256, 256, 1, 32, act, num_actions=3, embed=16, device="cuda").cuda()
        g = gen(5)
        B, T = 3, 4
        embed, action = dev(torch.randn(B, T, 16, generator=g)), dev(torch.randn(B, T, 3, generator=g))
        first = torch.zeros(B, T)
        first[:, 0] = 1
        ops.PROFILE.start()
        with torch.no_grad():
            post, _ = dyn.observe(embed, action, dev(first))
        keys[act] = set(ops.PROFILE.stop())
        assert torch.isfinite(post["deter"]).all()
    fused = "dv3_onehot_sample_linear_ln_fwd"
    assert fused in keys["SiLU"], sorted(keys["SiLU"])
    assert fused not in keys["ELU"] and "dv3_onehot_linear_ln_fwd" in keys["ELU"], sorted(keys["ELU"])
    # the C entry itself: code 3 is rejected before any launch
    lib = _lib.load()
    y = dev(torch.full((2, 256), 7.0))
    p = y.data_ptr()
    rc = lib.dv3_onehot_sample_linear_ln_fwd(p, p, 0, 0, p, 0, 0, 0, 0.01, 0, p, p, p, p, p, 4, 0, 0, 0, p, 256, p, 256, p, p, p,
                                             256, 0, 0, 2, 256, 3, ops._stream())
    assert rc == 10001
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 == float(y.max())


def _head_inputs(M, U, A, code, seed):
    g = gen(seed)
    pre = torch.randn(M, U, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(U, generator=g), 0.1 * torch.randn(U, generator=g)
    beta[3], beta[U - 2] = 40.0, -40.0
    if code == 2:
        for _ in range(50):
            bad = ln_act64(pre, gamma, beta, 0).abs() < 1e-3
            if not bad.any():
                break
            pre = pre + 0.05 * bad.float()
        assert not bad.any()
    Wm, Ws = torch.randn(A, U, generator=g) / math.sqrt(U), torch.randn(A, U, generator=g) / math.sqrt(U)
    bm, bs = 0.1 * torch.randn(A, generator=g), 0.1 * torch.randn(A, generator=g)
    return g, pre, gamma, beta, Wm, Ws, bm, bs


@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("U", [64, 130])
@pytest.mark.parametrize("code", CODES)
def test_actor_head_continuous_every_code(ops, code, U, A):
    M = 9
    g, pre, gamma, beta, Wm, Ws, bm, bs = _head_inputs(M, U, A, code, 1000 + 10 * U + A + code)
    eps = torch.randn(M, A, generator=g)
    y_ref = ln_act64(pre, gamma, beta, code)
    mr, sr = y_ref @ Wm.to(F64).t() + bm.to(F64), y_ref @ Ws.to(F64).t() + bs.to(F64)
    mu, sd = torch.tanh(mr), 0.9 * torch.sigmoid(sr + 2.0) + 0.1
    a = mu + sd * eps.to(F64)
    a_ref = a / torch.clip(a.abs(), min=1.0)
    ent_ref = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(sd)).sum(-1)
    mk = lambda *s: torch.full(s, 7.0, device="cuda")
    y, mean, rstd, om, os_, act, ent, eps_out = mk(M, U), mk(M), mk(M), mk(M, A), mk(M, A), mk(M, A), mk(M), mk(M, A)
    ops.actor_head(dev(pre), dev(gamma), dev(beta), y, mean, rstd, dev(Wm), dev(bm), dev(Ws), dev(bs), om, os_, act, ent,
                   noise=dev(eps), eps_out=eps_out, min_std=0.1, max_std=1.0, act=code)
    what = f"{NAMES[code]} U={U} A={A}"
    check(y, y_ref, what=what + " y")
    check(om, mr, what=what + " mean head"), check(os_, sr, what=what + " std head")
    check(act, a_ref, what=what + " action"), check(ent, ent_ref, what=what + " entropy")
    # the unfused pair: ln_act_fwd at the same code, then the two head Linears (the existing SiLU test's 1e-4)
    y_u, m_u, r_u, om_u, os_u = mk(M, U), mk(M), mk(M), mk(M, A), mk(M, A)
    ops.ln_act_fwd(dev(pre), dev(gamma), dev(beta), y_u, m_u, r_u, act=code)
    ops.gemm(y_u, dev(Wm), om_u, bias=dev(bm))
    ops.gemm(y_u, dev(Ws), os_u, bias=dev(bs))
    assert_close(y, y_u.cpu(), what=what + " y vs ln_act_fwd")
    assert_close(om, om_u.cpu(), what=what + " mean head vs gemm"), assert_close(os_, os_u.cpu(), what=what + " std head vs gemm")


@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("U", [64, 130])
@pytest.mark.parametrize("code", CODES)
def test_actor_head_onehot_every_code(ops, code, U, A):
    from oracle import dv3_oracle as O

    M = 9
    g, pre, gamma, beta, Wm, _, bm, _ = _head_inputs(M, U, A, code, 2000 + 10 * U + A + code)
    q = torch.empty(M, A).exponential_(1.0, generator=g).clamp_min(1e-20)
    y_ref = ln_act64(pre, gamma, beta, code)
    lg = y_ref @ Wm.to(F64).t() + bm.to(F64)
    ent_ref = O.onehot_entropy(lg[:, None, :], 0.01)
    mk = lambda *s: torch.full(s, 7.0, device="cuda")
    y, mean, rstd, om, act, ent = mk(M, U), mk(M), mk(M), mk(M, A), mk(M, A), mk(M)
    ai = torch.empty(M, dtype=torch.int32, device="cuda")
    ops.actor_head(dev(pre), dev(gamma), dev(beta), y, mean, rstd, dev(Wm), dev(bm), None, None, om, None, act, ent,
                   noise=dev(q), act_idx=ai, unimix=0.01, onehot=True, act=code)
    what = f"{NAMES[code]} onehot U={U} A={A}"
    check(y, y_ref, what=what + " y"), check(om, lg, what=what + " logits"), check(ent, ent_ref, what=what + " entropy")
    assert torch.equal(ai.cpu().long(), act.cpu().argmax(-1)) and act.sum(-1).eq(1).all()
    # the draw is the argmax of p_hat / q of the kernel's own logits
    samp = O.onehot_sample(om.cpu().double(), q.double(), 0.01)
    assert torch.equal(act.cpu().double(), samp)


@pytest.mark.parametrize("code", CODES)
def test_scan_ln_gemm_every_code(ops, code):
    """dv3_scan_ln_gemm_fwd(_ex) == ln_act_fwd + the few-row GEMM at the same code, bit-equal as the SiLU test asserts,
    and against float64."""
    M, K, N = 16, 256, 48
    x, gam, bet, _ = make_ln_inputs(M, K, code, True, 3000 + code, x_scale=2.0)
    g = gen(3100 + code)
    W, bias = torch.randn(N, K, generator=g) / math.sqrt(K), 0.1 * torch.randn(N, generator=g)
    xd, gd, bd, Wd, biasd = dev(x), dev(gam), dev(bet), dev(W), dev(bias)
    mk = lambda *s: torch.full(s, float("nan"), device="cuda")
    a = dict(y=mk(M, K), mean=mk(M), rstd=mk(M), C=mk(M, N))
    b = dict(y=mk(M, K), mean=mk(M), rstd=mk(M), C=mk(M, N))
    ops.ln_act_fwd(xd, gd, bd, a["y"], a["mean"], a["rstd"], act=code)
    ops.gemm(a["y"], Wd, a["C"], bias=biasd)
    ops.scan_ln_gemm(xd, gd, bd, b["y"], b["mean"], b["rstd"], Wd, b["C"], bias=biasd, act=code)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
    y_ref = ln_act64(x, gam, bet, code)
    check(b["y"], y_ref, what=f"{NAMES[code]} y")
    check(b["C"], y_ref @ W.to(F64).t() + bias.to(F64), tol=TOL * math.sqrt(K / 64), what=f"{NAMES[code]} C")


@pytest.mark.parametrize("code", CODES)
def test_scan_ln_factors_and_lnbwd_gemm_every_code(ops, code):
    """scan_ln_factors(act) + scan_lnbwd_gemm == ln_act_bwd(act) + the atomically accumulating data-gradient GEMM, to
    the tolerances of the SiLU test, and against float64 autograd."""
    M, K, N = 16, 256, 64
    x, gam, bet, dy = make_ln_inputs(M, K, code, True, 4000 + code)
    g = gen(4100 + code)
    W = torch.randn(K, N, generator=g) / math.sqrt(K)
    C0 = torch.randn(M, N, generator=g)
    xd, gd, bd, dyd, Wd = dev(x), dev(gam), dev(bet), dev(dy), dev(W)
    y, mean, rstd = torch.empty(M, K).cuda(), torch.empty(M).cuda(), torch.empty(M).cuda()
    ops.ln_act_fwd(xd, gd, bd, y, mean, rstd, act=code)
    a = dict(dx=torch.empty(M, K).cuda(), dg=torch.ones(K).cuda(), db=torch.ones(K).cuda(), C=dev(C0.clone()))
    b = dict(dx=torch.empty(M, K).cuda(), dg=torch.ones(K).cuda(), db=torch.ones(K).cuda(), C=dev(C0.clone()))
    ops.ln_act_bwd(dyd, xd, gd, bd, mean, rstd, a["dx"], a["dg"], a["db"], act=code)
    ops.gemm(a["dx"], Wd, a["C"], transB=False, accumulate="atomic")
    xhat, jac = torch.empty(M, K).cuda(), torch.empty(M, K).cuda()
    ops.scan_ln_factors(xd, gd, bd, mean, rstd, xhat, jac, act=code)
    ops.scan_lnbwd_gemm(dyd, xhat, jac, gd, rstd, b["dx"], Wd, b["C"], b["dg"], b["db"])
    assert_close(b["dx"], a["dx"].cpu(), tol=2e-6, what="dx")
    assert_close(b["dg"], a["dg"].cpu(), tol=1e-5, what="dgamma"), assert_close(b["db"], a["db"].cpu(), tol=1e-5, what="dbeta")
    assert_close(b["C"], a["C"].cpu(), tol=1e-5 * math.sqrt(K / 64), what="C")
    _, _, _, dx_ref, dg_ref, db_ref = ref_fwd_bwd(x, gam, bet, dy, code)
    z = ln_act64(x, gam, bet, 0).requires_grad_(True)
    (jac_ref,) = torch.autograd.grad(act64(z, code).sum(), z)
    what = NAMES[code]
    check(jac, jac_ref, what=what + " jac")
    check(b["dx"], dx_ref, what=what + " dx"), check(b["dg"] - 1, dg_ref, what=what + " dgamma")
    check(b["db"] - 1, db_ref, what=what + " dbeta")
    check(b["C"], C0.to(F64) + dx_ref @ W.to(F64), tol=TOL * math.sqrt(K / 64), what=what + " C")


@pytest.mark.parametrize("code", CODES)
def test_ens_ln_act_every_code(ops, code):
    """Member-batched LayerNorm + act, 3 members x 5 rows x 24 columns: against the per-member ln_act kernels at the
    same code (tolerances of test_member_indexed_layernorm_silu) and against float64."""
    K, M, U = 3, 5, 24
    xs, gs, bs, dys = zip(*(make_ln_inputs(M, U, code, True, 5000 + 10 * code + k) for k in range(K)))
    x, dy, g, b = dev(torch.stack(xs)), dev(torch.stack(dys)), dev(torch.stack(gs)), dev(torch.stack(bs))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(K * M, device="cuda"), torch.empty(K * M, device="cuda")
    dg, db = torch.zeros_like(g), torch.zeros_like(b)
    ops.ens_ln_act_fwd(x, g, b, y, mean, rstd, act=code)
    ops.ens_ln_act_bwd(dy, x, g, b, mean, rstd, dx, dg, db, act=code)
    dx2 = torch.empty_like(x)
    ops.ens_ln_act_bwd(dy, x, g, b, mean, rstd, dx2, act=code)  # without parameter gradients
    assert torch.equal(dx2, dx)
    for k in range(K):
        yk, dxk = torch.empty(M, U, device="cuda"), torch.empty(M, U, device="cuda")
        mk, rk = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        dgk, dbk = torch.zeros(U, device="cuda"), torch.zeros(U, device="cuda")
        gk, bk = g[k].contiguous(), b[k].contiguous()
        ops.ln_act_fwd(x[k], gk, bk, yk, mk, rk, act=code)
        ops.ln_act_bwd(dy[k], x[k], gk, bk, mk, rk, dxk, dgk, dbk, act=code)
        ens_close(y[k], yk, tol=1e-5, what=f"LN+act member {k}")
        ens_close(dx[k], dxk, tol=GTOL, what=f"dx member {k}")
        ens_close(dg[k], dgk, tol=GTOL, what=f"dgamma member {k}")
        ens_close(db[k], dbk, tol=GTOL, what=f"dbeta member {k}")
        y_ref, _, _, dx_ref, dg_ref, db_ref = ref_fwd_bwd(xs[k], gs[k], bs[k], dys[k], code)
        what = f"{NAMES[code]} member {k}"
        check(y[k], y_ref, what=what + " y"), check(dx[k], dx_ref, what=what + " dx")
        check(dg[k], dg_ref, what=what + " dgamma"), check(db[k], db_ref, what=what + " dbeta")


def test_layernorm_on_load_prologue_is_never_launched_for_a_layer(ops):
    """The one SiLU-only site, dv3_gemm_sample_f32's LayerNorm-on-load prologue, is bypassed: an imagination step of an
    ELU model runs ln_act_fwd (with the code) and hands the sampler the activated tensor."""
    import inspect

    from dv3hip import engine as E
    from tests.golden import act_common as AC
    from tests import helpers as Hh

    assert "ln=" not in inspect.getsource(E)
    cfg, wm, _ = Hh.build_models("tiny_elu", weights=AC.make_weights("tiny_elu"))
    M = 40  # (> 32 rows: the sampling epilogue's own range)
    dyn = wm.dynamics
    st = dyn.initial(M)
    ops.PROFILE.by_shape = False
    ops.PROFILE.start()
    with torch.no_grad():
        dyn.img_step(st, torch.zeros(M, cfg.num_actions, device="cuda"))
    rec = ops.PROFILE.stop()
    assert any(k.startswith("dv3_ln_act_fwd") for k in rec), list(rec)
    assert dyn.params().img_out.act == ops.ACT_CODES["ELU"] == dyn.params().img_in.act
