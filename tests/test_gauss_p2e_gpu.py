"""Plan2Explore on continuous latents (dyn_discrete: 0) through the fused route -- Plan2Explore.train_fwd_bwd +
train_opt: the member-batched ensemble kernels on [stoch | deter | action?] packed by ops.ens_pack_rows, the
disagreement as ImagBehavior's ensemble objective, the Gaussian reverse rollout -- against

* the REFERENCE's own exploration.Plan2Explore.train (tests/golden/tiny_gauss_p2e*.npz, written by
  tests/golden/make_golden_gauss_p2e.py) on the same weights, batch and N(0,1) draws;
* the autograd route (`train`) of this package from identical weights;
* hipGraph replay of the explorer half at agent level against eager launches;
* every disag_target (`feat` = [stoch | deter] is S + De wide);
and, as a control, the categorical `tiny_p2e` update: the parameters and the number of library launches of the
commit before the Gaussian route existed.

Bars.  Outputs, metrics and the intrinsic reward 1e-4; the exploration actor's and critic's gradients
tests/gauss_helpers.py's GRAD_TOL (5e-6 of the tensor's max); Adam-updated parameters gauss_helpers.adam_close (1e-6);
the ensemble's loss 1e-5, its gradients and gradient norm 3e-4 and its parameters adam_close at lr 1e-4 -- what
tests/test_p2e_fused_gpu.py holds the categorical fixtures to.  Every comparison prints its figure."""
import os

import numpy as np
import pytest
import torch

from tests import gauss_helpers as G
from tests import helpers as Hh
from tests.golden import common, gauss_common as GC, gauss_p2e_common as GP
from tests.test_autograd_gpu import GTOL
from tests.test_path_gpu import adam_close as ens_adam_close, close as ens_close

pytestmark = pytest.mark.gpu

ENS_LR, BEH_LR = 1e-4, 3e-5  # model_lr (the explorer's optimizer), actor / critic lr


def _build(name, target=None, weights=True):
    import exploration

    cfg, wm, _ = Hh.build_models(name, weights=GP.make_weights(name))
    if target is not None:
        cfg.disag_target = target
    extr = lambda f, st, a: wm.heads["reward"](f).mean()  # dreamer.py:80
    p2e = exploration.Plan2Explore(cfg, wm, extr).cuda()
    if weights:
        sd = p2e.state_dict()
        for k, v in GP.make_p2e_weights(name).items():
            assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
            sd[k] = torch.from_numpy(v)
            if k.startswith("_behavior.actor."):
                sd[k[len("_behavior."):]] = sd[k]
        p2e.load_state_dict(sd)
    p2e.requires_grad_(False)
    return cfg, wm, p2e


def _own_grads(p2e):
    return {k: v.grad.clone() for k, v in p2e.named_parameters()
            if v.grad is not None and not k.startswith(("_behavior._world_model", "actor."))}


def _update(name, fused, profile=False, target=None, state=None):
    """One world-model update, then one exploration update on its posterior -> dict(p2e, mets, grads[, launches])."""
    from dv3hip import ops

    cfg, wm, p2e = _build(name, target, weights=target is None)
    if state is not None:
        p2e.load_state_dict(state)
    start = {k: v.clone() for k, v in p2e.state_dict().items()}
    wm_noise, _ = G.gpu_noise(name)
    _, x_noise = G.gpu_noise(name, seed=GP.NOISE_SEED_X)
    data = GC.make_batch(name)
    post, context, _ = wm._train(data, noise=wm_noise)
    if profile:
        ops.PROFILE.start()
    if fused:
        assert p2e.fused_reason() is None and p2e.fused()
        p2e.train_fwd_bwd(post, context, data, noise=x_noise)
        _, mets = p2e.train_opt()
    else:
        stock = p2e._behavior._train
        p2e._behavior._train = lambda st, obj: stock(st, obj, noise=x_noise)
        _, mets = p2e.train(post, context, data)
    launches = ops.PROFILE.stop() if profile else None
    torch.cuda.synchronize()
    return dict(name=name, p2e=p2e, cfg=cfg, mets={k: float(v) for k, v in mets.items()}, grads=_own_grads(p2e),
                launches=launches, start=start)


@pytest.fixture(scope="module", params=GP.NAMES)
def fused_run(request):
    run = _update(request.param, fused=True, profile=True)
    run["g"] = G.gold(request.param)
    return run


def test_fused_ensemble_update_matches_the_reference(fused_run):
    g, mets, p2e = fused_run["g"], fused_run["mets"], fused_run["p2e"]
    print(f"[loss] explorer_loss {mets['explorer_loss']:.7f} vs {float(g['train/explorer_loss']):.7f}")
    ens_close(torch.tensor(mets["explorer_loss"]), torch.from_numpy(np.asarray(g["train/explorer_loss"])), tol=1e-5,
              what="explorer_loss")
    ens_close(torch.tensor(mets["explorer_grad_norm"]), torch.from_numpy(np.asarray(g["train/explorer_grad_norm"])),
              tol=GTOL, what="explorer_grad_norm")
    n = 0
    for k, gr in fused_run["grads"].items():
        if k.startswith("_networks."):
            ref = torch.from_numpy(g["grad/" + k])
            err = (gr.cpu().double() - ref.double()).abs().max().item()
            print(f"[ens grad] {k}: max err {err:.3e} tensor max {ref.abs().max().item():.3e}")
            ens_close(gr, ref, tol=GTOL, what="reference grad/" + k)
            n += 1
    assert n == sum(k.startswith("grad/_networks.") for k in g.files) > 0
    sd = p2e.state_dict()
    for k in sd:
        if k.startswith("_networks."):
            ens_adam_close(sd[k], torch.from_numpy(g["after/" + k]), ENS_LR, "after/" + k)
    # the inputs and the target were packed by the new kernel, one launch each, and no ATen route was taken
    la = fused_run["launches"]
    packs = sum(v["launches"] for k, v in la.items() if "dv3_ens_pack_rows" in k)
    assert packs == 3, {k: v["launches"] for k, v in la.items()}  # p2e.x, p2e.target, bh.ens_x


def test_fused_behaviour_update_matches_the_reference(fused_run):
    name, g, mets, p2e = fused_run["name"], fused_run["g"], fused_run["mets"], fused_run["p2e"]
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    beh = p2e._behavior
    unperm = lambda x: Hh.from_time_major_rows(x, B, T)
    G.close(unperm(beh._last["reward"]), g["imag/reward"].squeeze(-1), what="intrinsic reward")
    im = beh._im
    G.close(unperm(torch.cat([im["stoch"], im["deter"]], -1)), g["imag/feat"], what="imagined feat")
    G.close(unperm(im["action"]), g["imag/action"], what="imagined action")
    assert set(GP.TRAIN_KEYS) <= set(mets), set(GP.TRAIN_KEYS) - set(mets)
    for k in GP.TRAIN_KEYS:
        if not k.startswith("explorer_"):  # (losses 1e-5, the rest -- gradient norms too -- 1e-4: test_gauss_path_gpu.py)
            G.close(torch.tensor(mets[k]), g["train/" + k], tol=1e-5 if k.endswith("_loss") else G.TOL, what=k)
    n = 0
    for k, gr in fused_run["grads"].items():
        if k.startswith(("_behavior.actor.", "_behavior.value.")):
            G.grad_close(gr, g["grad/" + k], what="grad/" + k, tol=G.grad_tol(k[len("_behavior."):]))
            n += 1
    assert n == sum(k.startswith("grad/_behavior.") for k in g.files) > 0
    sd = p2e.state_dict()
    for k in sd:
        if k.startswith(("_behavior.actor.", "_behavior.value.")):
            G.adam_close(sd[k], g["after/" + k], BEH_LR, "after/" + k)
        elif k.startswith("_behavior._slow_value."):
            G.close(sd[k], g["after/" + k], tol=G.ADAM_TOL, what="after/" + k)
        elif k == "_behavior.ema_vals":
            G.close(sd[k], g["after/" + k], what="after/" + k)
    # the ensemble objective was never probed or evaluated as a foreign (autograd) objective
    assert not beh.__dict__.get("_objective_kinds")
    # the disagreement backward runs only with disag_action_cond (the objective sees the detached feat)
    bwd = [k for k in fused_run["launches"] if "disag_bwd" in k]
    assert bool(bwd) == bool(s["p2e"]["disag_action_cond"]), list(fused_run["launches"])


@pytest.mark.parametrize("name", GP.NAMES)
def test_fused_agrees_with_the_autograd_route(name, capfd):
    """The same update by `train` and fused, from identical weights and noise: the metric dict (keys and values) the
    agent prefixes with expl_, and every gradient."""
    a, f = _update(name, fused=False), _update(name, fused=True)
    assert "autograd route" not in capfd.readouterr().err
    assert set(a["mets"]) == set(f["mets"]), set(a["mets"]) ^ set(f["mets"])
    for k, v in a["mets"].items():
        if k == "explorer_loss":
            ens_close(torch.tensor(f["mets"][k]), torch.tensor(v), tol=1e-5, what=k)
        elif k == "explorer_grad_norm":
            ens_close(torch.tensor(f["mets"][k]), torch.tensor(v), tol=GTOL, what=k)
        else:
            G.close(torch.tensor(f["mets"][k]), torch.tensor(v), tol=1e-5 if k.endswith("_loss") else G.TOL, what=k)
    assert set(a["grads"]) == set(f["grads"])
    for k, v in a["grads"].items():
        if k.startswith("_networks."):
            ens_close(f["grads"][k], v, tol=GTOL, what="grad " + k)
        else:
            G.grad_close(f["grads"][k], v, what="grad " + k, tol=G.grad_tol(k[len("_behavior."):]))
    sa, sf = a["p2e"].state_dict(), f["p2e"].state_dict()
    for k in sa:
        if k.startswith("_networks."):
            ens_adam_close(sf[k], sa[k], ENS_LR, "after " + k)
        elif k.startswith(("_behavior.actor.", "_behavior.value.")):
            G.adam_close(sf[k], sa[k], BEH_LR, "after " + k)


@pytest.mark.parametrize("target", ["stoch", "deter", "embed", "feat"])
def test_every_disag_target_builds_and_trains(target):
    """One fused update per disag_target on the action-conditioned configuration (freshly initialised members), against
    the autograd route from the same weights; `feat` predicts [stoch | deter]."""
    name = "tiny_gauss_p2e_ac"
    s = common.SHAPES[name]
    f = _update(name, fused=True, target=target)
    a = _update(name, fused=False, target=target, state=f["start"])
    width = GP.target_width(name, target)
    if target == "feat":
        assert width == s["stoch"] + s["deter"]
    for net in f["p2e"]._networks:
        assert net.mean_layer.weight.shape[0] == width
        assert tuple(f["grads"]["_networks.0.mean_layer.bias"].shape) == (width,)
    assert all(np.isfinite(v) for v in f["mets"].values()), f["mets"]
    ens_close(torch.tensor(f["mets"]["explorer_loss"]), torch.tensor(a["mets"]["explorer_loss"]), tol=1e-5,
              what=f"explorer_loss ({target})")
    for k, v in a["grads"].items():
        if k.startswith("_networks."):
            ens_close(f["grads"][k], v, tol=GTOL, what=f"grad {k} ({target})")


def _agent(name, seed=0, **over):
    import dreamer
    import tools

    tools.set_seed_everywhere(seed)
    cfg = Hh.make_config(name)
    cfg.log_every, cfg.train_ratio, cfg.reset_every, cfg.expl_until, cfg.action_repeat = 1e9, 1, 0, 0, 1
    cfg.pretrain, cfg.video_pred_log = 1, False
    for k, v in over.items():
        setattr(cfg, k, v)
    agent = dreamer.Dreamer(Hh.obs_space(name), None, cfg, None, None).cuda()
    agent.requires_grad_(False)
    return agent


def test_agent_replays_the_gaussian_explorer(capfd):
    """dreamer.Dreamer with expl_behavior plan2explore and dyn_discrete 0: UpdateRunner.attach_explorer takes the explorer,
    captures its three graphs after the warm-up and replays them; an agent at hip_graph=False fed the same batches
    (eager launches) reaches the same explorer losses (compared as tests/test_p2e_fused_gpu.py compares them)."""
    name = "tiny_gauss_p2e_ac"
    seqs, agents = {}, {}
    for graph in (True, False):
        agent = _agent(name, hip_graph=graph)
        if not graph:
            agent.load_state_dict(start)
        else:
            start = {k: v.clone() for k, v in agent.state_dict().items()}
        for i in range(5):
            agent._train(GC.make_batch(name, seed=i))
            agent._flush_metrics()  # (one entry per update in every metric's list)
        seqs[graph], agents[graph] = dict(agent._metrics), agent
    ga = agents[True]
    r = ga._runner
    assert ga._expl_behavior.fused()
    assert r.use_graph and r.expl is ga._expl_behavior and r._g_expl is not None and len(r._g_expl) == 3
    assert agents[False]._runner._g_expl is None
    err = capfd.readouterr().err
    assert "autograd route" not in err and "capture refused" not in err, err
    keys = {k for k in seqs[True] if k.startswith("expl_")}
    for k in ("expl_explorer_loss", "expl_explorer_grad_norm", "expl_actor_loss", "expl_value_loss", "expl_imag_reward_mean",
              "expl_actor_grad_norm", "expl_value_grad_norm", "expl_actor_entropy"):
        assert k in keys, (k, sorted(keys))
    assert keys == {k for k in seqs[False] if k.startswith("expl_")}
    for k in keys:
        assert len(seqs[True][k]) == 5 and np.all(np.isfinite(seqs[True][k])), (k, seqs[True][k])
    print("[replay] explorer loss", seqs[True]["expl_explorer_loss"], "eager", seqs[False]["expl_explorer_loss"])
    ens_close(torch.tensor(seqs[True]["expl_explorer_loss"]), torch.tensor(seqs[False]["expl_explorer_loss"]), tol=1e-5,
              what="explorer loss over 5 updates, replay vs eager")
    G.close(torch.tensor(seqs[True]["expl_imag_reward_mean"]), torch.tensor(seqs[False]["expl_imag_reward_mean"]),
            what="intrinsic reward mean over 5 updates, replay vs eager")
    b = ga._expl_behavior._expl_opt.bucket.ensure()
    assert b.members == common.SHAPES[name]["p2e"]["disag_models"]


# ---------------------------------------------------------------------------------------------
# control: the categorical route is what it was
# ---------------------------------------------------------------------------------------------
# ops.PROFILE's launch count of one fused tiny_p2e exploration update (train_fwd_bwd + train_opt), and the parameters
# after it (tests/golden/tiny_p2e_fused_parent.npz), both recorded on an MI355X from the commit before this route
# (tests/golden/make_p2e_parent_control.py).  The first Adam step moves a parameter by lr g / (|g| + eps): the order of
# the LayerNorm gradients' atomic adds cannot reach the stored bits, and two runs of the recording agreed bit for bit.
PARENT_LAUNCHES = 153


def test_categorical_update_is_unchanged():
    from tests.test_p2e_fused_gpu import _update as cat_update

    run = cat_update("tiny_p2e", fused=True, profile=True)
    la = run["launches"]
    assert not any("ens_pack_rows" in k for k in la), list(la)
    total = sum(v["launches"] for v in la.values())
    print(f"[control] tiny_p2e fused update: {total} library launches")
    assert total == PARENT_LAUNCHES
    ref = np.load(os.path.join(G.GOLDEN, "tiny_p2e_fused_parent.npz"), allow_pickle=False)
    sd = run["p2e"].state_dict()
    own = [k for k in sd if not k.startswith(("_behavior._world_model.", "actor."))]
    assert set(own) == set(ref.files), set(own) ^ set(ref.files)
    for k in own:
        assert np.array_equal(sd[k].cpu().numpy(), ref[k]), k
