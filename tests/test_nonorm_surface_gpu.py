"""norm / encoder.norm / decoder.norm: False on the device, beside the reference parity of tests/test_nonorm_path_gpu.py:

  * a reference-format checkpoint (the fixture weights under the reference's names) loads with strict=True and the
    optimizers' state_dict round-trips;
  * networks.MLP(norm=False) and networks.GRUCell(norm=False) forward and backward through dv3hip.autograd against
    float64 torch on the CPU with the same weights, at 1e-4 * max(1, max|ref|) -- the route Plan2Explore's objective
    and every other `loss.backward()` caller takes;
  * a Plan2Explore config with norm: False constructs, takes the autograd route for a reason that names `norm`, and
    one exploration update there gives finite metrics and moves every ensemble parameter;
  * the choice of a fused launch is per layer: encoder.norm False with norm True keeps the RSSM's and the actor's
    LayerNorm fusions, norm False drops exactly those and keeps the ones without a LayerNorm;
  * at a width where the observe scan fuses the next step's reset blend into the GRU launch and gathers weight columns
    for the one-hot input (deter = hidden = 256, 32 classes), RSSM.observe without LayerNorm equals the step-by-step
    obs_step chain, which takes neither."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as Hh
from tests import nonorm_helpers as N
from tests.golden import common
from tests.golden import nonorm_common as NC

pytestmark = pytest.mark.gpu
TOL = 1e-4


def check(got, ref, what, tol=TOL):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err, bar = (got - ref).abs().max().item(), tol * max(1.0, ref.abs().max().item())
    print(f"{what}: max err {err:.3e} bar {bar:.3e}")
    assert err <= bar, f"{what}: max err {err:.3e} > bar {bar:.3e}"


@pytest.mark.parametrize("name", NC.NAMES)
def test_reference_format_checkpoint_loads_strictly(name):
    import dreamer
    from tests.test_nonorm_path_gpu import _Logger

    cfg = Hh.make_config(name)
    cfg.pretrain = 0
    cfg.expl_behavior = "greedy"
    agent = dreamer.Dreamer(Hh.obs_space(name), None, cfg, _Logger(), iter(())).to(cfg.device)
    w = NC.make_weights(name)
    sd, used = agent.state_dict(), set()
    for k in sd:  # the reference's agent_state_dict names (dreamer.py: _wm.*, _task_behavior.*[_world_model.*])
        key = k
        for pre in ("_wm.", "_task_behavior.", "_expl_behavior.", "_world_model."):  # (greedy: the explorer is the task behaviour)
            if key.startswith(pre):
                key = key[len(pre):]
        if key == "ema_vals":
            continue
        assert key in w, f"{k}: not a name of the reference's checkpoint"
        assert tuple(sd[k].shape) == w[key].shape, (k, sd[k].shape, w[key].shape)
        sd[k] = torch.from_numpy(w[key])
        used.add(key)
    assert used == set(w), sorted(set(w) - used)
    agent.load_state_dict(sd, strict=True)
    now = agent.state_dict()
    for k, v in w.items():
        pre = "_wm." if k.split(".")[0] in Hh.WM_PREFIXES else "_task_behavior."
        assert torch.equal(now[pre + k].cpu(), torch.from_numpy(v)), k
    # optimizer state: one update, then state_dict -> load_state_dict -> state_dict is the identity
    data = NC.make_batch(name)
    post, _, _ = agent._wm._train_eager(data)
    agent._task_behavior._train_eager(post)
    for opt in (agent._wm._model_opt, agent._task_behavior._actor_opt, agent._task_behavior._value_opt):
        sd = opt.state_dict()
        assert len(sd["state"]) == len(opt._opt.param_groups[0]["params"]) > 0
        opt.load_state_dict(sd)
        sd2 = opt.state_dict()
        assert sd["param_groups"] == sd2["param_groups"]
        for i, e in sd["state"].items():
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(e[key], sd2["state"][i][key]), (i, key)


@pytest.mark.parametrize("act", ["SiLU", "ELU"])
@pytest.mark.parametrize("rows,inp,units,layers", [(7, 5, 16, 2), (33, 36, 24, 3), (130, 64, 256, 1)])
def test_mlp_without_norm_matches_float64_torch(rows, inp, units, layers, act):
    import networks

    torch.manual_seed(rows)
    with networks.layernorm_free():
        mlp = networks.MLP(inp, None, layers, units, act=act, norm=False, name="T").cuda()
    assert [n for n, _ in mlp.layers.named_children()] == [f"T_{k}{i}" for i in range(layers) for k in ("linear", "act")]
    assert list(mlp.state_dict()) == [f"layers.T_linear{i}.weight" for i in range(layers)]
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    x, up = torch.randn(rows, inp), torch.randn(rows, units)
    # float64 reference
    ws = [getattr(mlp.layers, f"T_linear{i}").weight.detach().cpu().double().requires_grad_(True) for i in range(layers)]
    xd = x.double().requires_grad_(True)
    h = xd
    for W in ws:
        h = getattr(F, act.lower())(h @ W.t())
    ref = torch.autograd.grad(h, [xd] + ws, up.double())
    # the public class under autograd (dv3hip.autograd.TrunkFn over engine.MLPEngine)
    xg = x.cuda().requires_grad_(True)
    got_h = mlp(xg)
    assert got_h.requires_grad
    got = torch.autograd.grad(got_h, [xg] + [getattr(mlp.layers, f"T_linear{i}").weight for i in range(layers)], up.cuda())
    check(got_h, h, f"mlp output rows={rows} units={units}")
    for g, r, nm in zip(got, ref, ["dx"] + [f"dW{i}" for i in range(layers)]):
        check(g, r, f"mlp {nm} rows={rows} units={units}")
    # and without gradients (the forward-only engine route)
    with torch.no_grad():
        check(mlp(x.cuda()), h, "mlp output, no grad")


@pytest.mark.parametrize("M,inp,size", [(1, 4, 3), (5, 16, 16), (17, 256, 256)])
def test_gru_cell_without_norm_matches_float64_torch(M, inp, size):
    import networks

    torch.manual_seed(M)
    with networks.layernorm_free():
        cell = networks.GRUCell(inp, size, norm=False).cuda()
    assert list(cell.state_dict()) == ["layers.GRU_linear.weight"]
    x, h, up = torch.randn(M, inp), torch.tanh(torch.randn(M, size)), torch.randn(M, size)
    W = cell.layers.GRU_linear.weight.detach().cpu().double().requires_grad_(True)
    xd, hd = x.double().requires_grad_(True), h.double().requires_grad_(True)
    r, c, u = (torch.cat([xd, hd], -1) @ W.t()).chunk(3, -1)
    r = torch.sigmoid(r)
    c = torch.tanh(r * c)
    u = torch.sigmoid(u - 1)
    out = u * c + (1 - u) * hd
    ref = torch.autograd.grad(out, [xd, hd, W], up.double())
    xg, hg = x.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
    got_out, _ = cell(xg, [hg])
    got = torch.autograd.grad(got_out, [xg, hg, cell.layers.GRU_linear.weight], up.cuda())
    check(got_out, out, f"gru h' {M}x{size}")
    for g, r_, nm in zip(got, ref, ("dx", "dh", "dW")):
        check(g, r_, f"gru {nm} {M}x{size}")
    with torch.no_grad():
        check(cell(x.cuda(), [h.cuda()])[0], out, "gru h', no grad")


def test_plan2explore_without_norm_trains_on_the_autograd_route():
    import exploration
    import models

    name = "tiny_p2e"
    torch.manual_seed(0)
    cfg = Hh.make_config(name)
    cfg.norm = False
    wm = models.WorldModel(Hh.obs_space(name), None, 0, cfg).cuda()
    p2e = exploration.Plan2Explore(cfg, wm, lambda f, st, a: wm.heads["reward"](f).mean()).cuda()
    assert not p2e.fused() and "norm" in p2e.fused_reason()
    before = {k: v.detach().clone() for k, v in p2e._networks.named_parameters()}
    data = common.make_batch(name)
    post, context, _ = wm._train_eager(data)
    _, mets = p2e.train(post, context, data)
    torch.cuda.synchronize()
    assert mets and all(np.isfinite(float(v)) for v in mets.values()), mets
    assert float(mets["explorer_loss"]) != 0.0
    for k, v in p2e._networks.named_parameters():
        assert not torch.equal(v.detach(), before[k]), f"ensemble parameter {k} did not move"


def _wide(norm, enc_norm, B=2, T=4, H=3):
    """A model wide enough for every fused launch of the scans (hidden = deter = units = 256, 32 x 32 latents)."""
    import models

    torch.manual_seed(3)
    cfg = Hh.make_config("cfg2")
    cfg.norm, cfg.encoder["norm"] = norm, enc_norm
    cfg.dyn_hidden = cfg.dyn_deter = cfg.units = 256
    cfg.encoder["cnn_depth"] = cfg.decoder["cnn_depth"] = 4
    cfg.batch_size, cfg.batch_length, cfg.imag_horizon = B, T, H
    wm = models.WorldModel(Hh.obs_space("cfg2"), None, 0, cfg).cuda()
    beh = models.ImagBehavior(cfg, wm).cuda()
    rs = np.random.RandomState(0)
    first = np.zeros((B, T), bool)
    first[:, 0] = True
    data = dict(image=rs.randint(0, 256, size=(B, T, 64, 64, 3)).astype(np.uint8),
                action=rs.uniform(-1, 1, size=(B, T, cfg.num_actions)).astype(np.float32),
                reward=rs.randn(B, T).astype(np.float32), discount=np.ones((B, T), np.float32), is_first=first,
                is_terminal=np.zeros((B, T), bool))
    return cfg, wm, beh, data


def _launches(norm, enc_norm):
    from dv3hip import ops

    cfg, wm, beh, data = _wide(norm, enc_norm)
    ops.PROFILE.by_shape = False
    ops.PROFILE.start()
    post, _, mets = wm._train_eager(data)
    beh._train_eager(post)
    rec = ops.PROFILE.stop()
    assert np.isfinite(float(mets["model_loss"]))
    return {k: v["launches"] for k, v in rec.items()}


NAMED = ("gemm_kernel<skinny16+ln,tA=0,tB=1>", "dv3_onehot_sample_linear_ln_fwd", "dv3_actor_head_fwd")  # scan_ln_gemm, ...
LN_FUSIONS = NAMED + ("gemm_kernel<skinny16+lnbwd,tA=0,tB=0>", "dv3_scan_ln_factors", "dv3_scan_gru_factors")


def test_fusions_are_chosen_per_layer():
    base = _launches(True, True)
    for k in NAMED:
        assert base.get(k, 0) > 0, (k, sorted(base))
    assert not any(k.startswith(("dv3_act_", "dv3_gru_nonorm")) for k in base), sorted(base)
    # encoder.norm False, norm True: the conv stack loses its LayerNorm, the RSSM and the actor keep every fusion
    enc = _launches(True, False)
    for k in LN_FUSIONS + ("dv3_gru_fwd", "dv3_gru_bwd"):
        assert enc.get(k, 0) == base.get(k, 0), (k, enc.get(k, 0), base.get(k, 0))
    assert enc["dv3_act_fwd"] == 4 and enc["dv3_act_bwd"] == 4  # the four conv layers
    assert not any(k.startswith("dv3_gru_nonorm") for k in enc)
    # norm False, encoder.norm True: exactly the LayerNorm fusions go, the ones without a LayerNorm stay
    no = _launches(False, True)
    for k in LN_FUSIONS + ("dv3_gru_fwd", "dv3_gru_bwd"):
        assert k not in no, k
    assert no["dv3_gru_nonorm_fwd"] > 0 and no["dv3_gru_nonorm_bwd"] > 0 and no["dv3_act_fwd"] > 0
    k = "gemm_kernel<skinny16+carry_st,tA=0,tB=0>"
    assert no.get(k, 0) == base.get(k, 0), (no.get(k, 0), base.get(k, 0))
    assert no.get("dv3_onehot_linear_ln_fwd", 0) > 0, sorted(no)  # the one-hot gather (it writes pre; act_fwd follows)


def test_observe_scan_without_norm_equals_the_step_chain():
    """deter = hidden = 256, 32 classes: the scan takes gru_nonorm_fwd_blend and the one-hot gather followed by
    act_fwd; obs_step blends with reset_blend and multiplies the dense one-hot."""
    import networks
    from dv3hip import ops

    torch.manual_seed(1)
    S, D, B, T, A, Em = 4, 32, 3, 5, 3, 16
    with networks.layernorm_free():
        dyn = networks.RSSM(S, 256, 256, 1, D, "SiLU", False, num_actions=A, embed=Em, device="cuda").cuda()
    with torch.no_grad():
        dyn.W.copy_(0.5 * torch.randn_like(dyn.W))
    embed, action = torch.randn(B, T, Em).cuda(), torch.randn(B, T, A).cuda()
    first = torch.zeros(B, T)
    first[:, 0] = 1
    first[1, 2] = 1
    first = first.cuda()
    qp = torch.empty(T, B, S, D).exponential_().clamp_min(1e-20).cuda()
    qq = torch.empty(T, B, S, D).exponential_().clamp_min(1e-20).cuda()
    ops.PROFILE.by_shape = False
    ops.PROFILE.start()
    with torch.no_grad():
        post, prior = dyn.observe(embed, action, first, noise=dict(q_prior=qp, q_post=qq))
    rec = ops.PROFILE.stop()
    assert rec["dv3_gru_nonorm_fwd"]["launches"] == T and "dv3_gru_fwd" not in rec
    assert rec["dv3_act_fwd"]["launches"] >= 2 * T  # img_in and obs_out of every step (+ the batched prior head)
    state = None
    with torch.no_grad():
        for t in range(T):
            st, pr = dyn.obs_step(state, action[:, t] if t else None, embed[:, t], first[:, t],
                                  noise=dict(prior=qp[t], post=qq[t]))
            state = st
            for k in ("stoch", "deter", "logit"):
                if k == "stoch":
                    assert torch.equal(st[k], post[k][:, t]), f"step {t}: sampled classes differ"
                else:
                    check(st[k], post[k][:, t], f"post/{k}[{t}]", tol=1e-5)
            check(pr["logit"], prior["logit"][:, t], f"prior/logit[{t}]", tol=1e-5)
