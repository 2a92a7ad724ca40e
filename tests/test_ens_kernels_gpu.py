"""Member-batched ensemble kernels (csrc/ensops.hip, dv3hip.ops.ens_*, dv3hip.engine.EnsembleEngine) against float64
references on the CPU built from the oracle's Plan2Explore functions (oracle/dv3_oracle.py: p2e_member_mean,
p2e_ensemble_loss, p2e_intrinsic_reward) and their autograd.  Values 1e-4, gradients GTOL = 3e-4 of the tensor's scale
(the tolerances of tests/test_autograd_gpu.py).

Shapes: the smallest at which the kernels can go wrong -- fewer rows than one 64-row tile, rows / widths that are no tile
multiple, more than one workgroup per member, 2 / 3 / 10 members, and the stock widths (400 units, 1536 inputs, 1024
outputs) once."""
import zlib

import numpy as np
import pytest
import torch

from oracle import dv3_oracle as O
from tests.test_path_gpu import close

pytestmark = pytest.mark.gpu
GTOL = 3e-4

# (members, rows, layers, units, input width, action width inside it, target width)
CASES = {
    "k2_m15": dict(K=2, M=15, L=2, U=16, F=32, A=0, W=16),
    "k3_m72_action": dict(K=3, M=72, L=2, U=24, F=35, A=3, W=40),
    "k10_m130_stock": dict(K=10, M=130, L=4, U=400, F=1536, A=0, W=1024),
}


def _weights(c, seed=3):
    """Weights of K members drawn as tests/golden/common.make_p2e_weights draws them (one numpy stream per state_dict
    name), for free shapes."""
    out = {}
    for i in range(c["K"]):
        shapes = {}
        for j in range(c["L"]):
            shapes[f"_networks.{i}.layers.NoName_linear{j}.weight"] = (c["U"], c["F"] if j == 0 else c["U"])
            shapes[f"_networks.{i}.layers.NoName_norm{j}.weight"] = (c["U"],)
            shapes[f"_networks.{i}.layers.NoName_norm{j}.bias"] = (c["U"],)
        shapes[f"_networks.{i}.mean_layer.weight"] = (c["W"], c["U"])
        shapes[f"_networks.{i}.mean_layer.bias"] = (c["W"],)
        for k, shp in shapes.items():
            rs = np.random.RandomState((zlib.crc32(k.encode()) + 7919 * seed) & 0x7FFFFFFF)
            if len(shp) == 1:
                w = (1.0 + 0.1 * rs.randn(*shp)) if k.endswith(".weight") and "norm" in k else 0.1 * rs.randn(*shp)
            else:
                w = rs.randn(*shp) * np.sqrt(2.0 / (shp[0] + shp[1]))
            out[k] = w.astype(np.float32)
    return out


def _engine(c, w, *, scale=1.0, log=True):
    """EnsembleEngine over a member-major ParamBucket holding `w` (parameters in nn.ModuleList order)."""
    from dv3hip import engine as E
    from dv3hip.params import ParamBucket

    params = [torch.nn.Parameter(torch.from_numpy(v).cuda(), requires_grad=False) for v in w.values()]
    bucket = ParamBucket("ens_test", params, members=c["K"]).ensure()
    eng = E.EnsembleEngine("ens_test", bucket, c["L"], E.Workspace(torch.device("cuda")), std=O.P2E_STD, scale=scale,
                           log=log)
    return eng, bucket, dict(zip(w.keys(), params))


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    """Inputs and the float64 CPU reference of one shape, computed once and shared (never modified)."""
    c = CASES[request.param]
    rs = np.random.RandomState(11)
    w = _weights(c)
    x = rs.randn(c["M"], c["F"]).astype(np.float32)
    target = np.tanh(rs.randn(c["M"], c["W"])).astype(np.float32)
    drew = rs.randn(c["M"], 1).astype(np.float32)
    pc = O.P2EConfig(disag_models=c["K"], disag_layers=c["L"], disag_units=c["U"], disag_offset=0,
                     disag_action_cond=bool(c["A"]))
    pp = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w.items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    feat, act = (xd[:, :-c["A"]], xd[:, -c["A"]:]) if c["A"] else (xd, None)
    mu = torch.stack([O.p2e_member_mean(pc, pp, i, xd) for i in range(c["K"])], 0)
    loss = O.p2e_ensemble_loss(pc, pp, xd[None], torch.from_numpy(target).double()[None])
    grads = dict(zip(pp, torch.autograd.grad(loss, list(pp.values()))))
    ref = dict(mu=mu.detach(), loss=loss.detach(), grads=grads, rew={}, dx={})
    for log, scale in ((True, 1.0), (False, 0.7), (True, 0.7)):
        pcl = O.P2EConfig(disag_models=c["K"], disag_layers=c["L"], disag_units=c["U"], disag_offset=0,
                          disag_action_cond=bool(c["A"]), disag_log=log, expl_intr_scale=scale)
        r = O.p2e_intrinsic_reward(pcl, pp, feat, act)
        ref["rew"][(log, scale)] = r.detach()
        ref["dx"][(log, scale)] = torch.autograd.grad((r * torch.from_numpy(drew).double()).sum(), xd)[0]
    # the backward divides by the std over members: it must be well away from zero in the REFERENCE
    ref["min_std"] = float(mu.detach().std(0).min())
    ref["mu_scale"] = float(mu.detach().abs().max())
    return dict(c=c, w=w, x=x, target=target, drew=drew, ref=ref)


def test_reference_disagreement_is_well_conditioned(case):
    assert case["ref"]["min_std"] > 1e-4 * case["ref"]["mu_scale"], case["ref"]["min_std"]


def test_batched_gemm_forward_and_data_gradient(case):
    from dv3hip import ops

    c = case["c"]
    K, M, U, F = c["K"], c["M"], c["U"], c["F"]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(case["x"]).cuda()
    W = torch.from_numpy((rs.randn(K, U, F) / np.sqrt(F)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.randn(K, U).astype(np.float32)).cuda()
    dy = torch.from_numpy(rs.randn(K, M, U).astype(np.float32)).cuda()
    xd, Wd, dyd = x.cpu().double(), W.cpu().double(), dy.cpu().double()
    # forward, ONE shared input
    y = torch.full((K, M, U), float("nan"), device="cuda")
    ops.ens_gemm(x, W, y, bias=bias)
    ref_y = torch.stack([xd @ Wd[k].t() + bias[k].cpu().double() for k in range(K)])
    close(y, ref_y, what="y = x W_k^T + b_k (shared x)")
    # ... equals K replicated copies
    y_rep = torch.empty_like(y)
    ops.ens_gemm(x[None].repeat(K, 1, 1).contiguous(), W, y_rep, bias=bias)
    assert torch.equal(y, y_rep)
    # data gradient per member, and summed over members
    dx_k = torch.full((K, M, F), float("nan"), device="cuda")
    ops.ens_gemm(dy, W, dx_k, transB=False)
    ref_dx = torch.stack([dyd[k] @ Wd[k] for k in range(K)])
    close(dx_k, ref_dx, what="dx_k = dy_k W_k")
    dx = torch.full((M, F), float("nan"), device="cuda")
    ops.ens_gemm(dy, W, dx, transB=False)
    close(dx, ref_dx.sum(0), what="dx = sum_k dy_k W_k")
    close(dx, dx_k.sum(0), tol=1e-5, what="summed dx against the sum of the per-member ones")
    # weight gradient (accumulating, shared input)
    gW = torch.ones_like(W)
    ops.ens_gemm(dy, x, gW, transA=True, transB=False, accumulate=True)
    close(gW, torch.stack([dyd[k].t() @ xd for k in range(K)]) + 1.0, tol=GTOL, what="dW_k += dy_k^T x")
    gb = torch.zeros_like(bias)
    ops.ens_colsum(dy, gb)
    close(gb, dyd.sum(1), tol=GTOL, what="db_k = colsum dy_k")


def test_member_indexed_layernorm_silu(case):
    from dv3hip import ops

    c = case["c"]
    K, M, U = c["K"], c["M"], c["U"]
    rs = np.random.RandomState(6)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).cuda()
    x, dy = t(K, M, U), t(K, M, U)
    g, b = 1.0 + 0.1 * t(K, U), 0.1 * t(K, U)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(K * M, device="cuda"), torch.empty(K * M, device="cuda")
    dg, db = torch.zeros_like(g), torch.zeros_like(b)
    ops.ens_ln_act_fwd(x, g, b, y, mean, rstd)
    ops.ens_ln_act_bwd(dy, x, g, b, mean, rstd, dx, dg, db)
    for k in range(K):
        yk, dxk = torch.empty(M, U, device="cuda"), torch.empty(M, U, device="cuda")
        mk, rk = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        dgk, dbk = torch.zeros(U, device="cuda"), torch.zeros(U, device="cuda")
        gk, bk = g[k].contiguous(), b[k].contiguous()
        ops.ln_act_fwd(x[k], gk, bk, yk, mk, rk)
        ops.ln_act_bwd(dy[k], x[k], gk, bk, mk, rk, dxk, dgk, dbk)
        close(y[k], yk, tol=1e-5, what=f"LN+SiLU member {k}")
        close(mean[k * M:(k + 1) * M], mk, tol=1e-5, what="mean")
        close(rstd[k * M:(k + 1) * M], rk, tol=1e-5, what="rstd")
        close(dx[k], dxk, tol=GTOL, what=f"dx member {k}")
        close(dg[k], dgk, tol=GTOL, what=f"dgamma member {k}")
        close(db[k], dbk, tol=GTOL, what=f"dbeta member {k}")


def test_engine_forward_and_regression(case):
    c, ref = case["c"], case["ref"]
    eng, bucket, params = _engine(c, case["w"])
    x, target = torch.from_numpy(case["x"]).cuda(), torch.from_numpy(case["target"]).cuda()
    close(eng.forward(x), ref["mu"], what="member means")
    bucket.zero_grad()
    loss = eng.regress_fwd_bwd(x, target)
    close(loss, ref["loss"], tol=1e-5, what="ensemble loss")
    for k, p in params.items():
        close(p.grad, ref["grads"][k], tol=GTOL, what="grad " + k)
    # a second call reuses the loss kernel's ticket: same scalar
    bucket.zero_grad()
    assert float(eng.regress_fwd_bwd(x, target)) == float(loss)


@pytest.mark.parametrize("log,scale", [(True, 1.0), (False, 0.7), (True, 0.7)])
def test_disagreement_forward_and_backward(case, log, scale):
    c, ref = case["c"], case["ref"]
    eng, _, _ = _engine(c, case["w"], scale=scale, log=log)
    x = torch.from_numpy(case["x"]).cuda()
    r_nokeep = eng.disag_fwd(x, keep=False).clone()
    r = eng.disag_fwd(x, keep=True)
    close(r, ref["rew"][(log, scale)], what="intrinsic reward")
    assert torch.equal(r, r_nokeep)
    dx = eng.disag_bwd(torch.from_numpy(case["drew"]).cuda())
    close(dx, ref["dx"][(log, scale)], tol=GTOL, what="d reward / d input")


def test_single_member_is_rejected_without_a_launch():
    """K = 1: DV3_ERR_ARG, and no kernel ran -- every output still holds its sentinel afterwards."""
    from dv3hip import _lib, ops

    M, U, W = 15, 16, 16
    z = lambda *s: torch.zeros(*s, device="cuda")
    full = lambda *s: torch.full(s, 7.0, device="cuda")
    reward, disag, part, mu = full(M, 1), full(M), full(M), full(1, M, W)
    with pytest.raises(_lib.DV3Error, match="DV3_ERR_ARG"):
        ops.ens_disag_fwd(z(1, M, U), z(1, W, U), z(1, W), reward, disag, part, mu=mu)
    with pytest.raises(_lib.DV3Error, match="DV3_ERR_ARG"):
        ops.ens_disag_bwd(mu, disag, z(M, 1))
    torch.cuda.synchronize()
    for t in (reward, disag, part, mu):
        assert bool((t == 7.0).all())


def test_launch_count_does_not_grow_with_members():
    counts = {}
    for K in (2, 10):
        c = dict(K=K, M=72, L=2, U=24, F=32, A=0, W=40)
        eng, _, _ = _engine(c, _weights(c))
        x = torch.from_numpy(np.random.RandomState(1).randn(c["M"], c["F"]).astype(np.float32)).cuda()
        eng.disag_fwd(x)  # (allocates the workspace)
        from dv3hip import ops

        ops.PROFILE.start()
        eng.disag_fwd(x)
        counts[K] = sum(v["launches"] for v in ops.PROFILE.stop().values())
    assert counts[2] == counts[10] == 2 * 2 + 1, counts
