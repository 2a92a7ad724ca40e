"""exploration.Plan2Explore.train_fwd_bwd + train_opt: the exploration update without torch autograd (member-batched
ensemble kernels, the disagreement as ImagBehavior's ensemble objective) against

* the reference's own exploration.Plan2Explore.train (tests/golden/tiny_p2e*.npz) and the CPU oracle -- every comparison
  tests/test_autograd_gpu.py makes for the autograd route, with its tolerances, on the same weights, batch and noise;
* the autograd route (`train`) of this package from identical weights;
* at agent level: dreamer.Dreamer replaying the explorer half from hipGraphs against eager launches."""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests.golden import common
from tests.test_autograd_gpu import GTOL, _build_p2e, _gold
from tests.test_path_gpu import adam_close, close, gpu_noise

pytestmark = pytest.mark.gpu


def _update(name, fused, profile=False):
    """One world-model update, then one exploration update on its posterior -> dict(p2e, mets, grads[, launches])."""
    from dv3hip import ops

    cfg, wm, _ = Hh.build_models(name)
    p2e = _build_p2e(name, wm, cfg)
    wm_noise, _ = gpu_noise(name)
    _, x_noise = gpu_noise(name, seed=5)
    data = common.make_batch(name)
    post, context, _ = wm._train(data, noise=wm_noise)
    if profile:
        ops.PROFILE.start()
    if fused:
        assert p2e.fused()
        p2e.train_fwd_bwd(post, context, data, noise=x_noise)
        _, mets = p2e.train_opt()
    else:
        stock = p2e._behavior._train
        p2e._behavior._train = lambda st, obj: stock(st, obj, noise=x_noise)
        _, mets = p2e.train(post, context, data)
    launches = ops.PROFILE.stop() if profile else None
    torch.cuda.synchronize()
    grads = {k: v.grad.clone() for k, v in p2e.named_parameters()
             if v.grad is not None and not k.startswith(("_behavior._world_model", "actor."))}
    return dict(name=name, p2e=p2e, mets={k: float(v) for k, v in mets.items()}, grads=grads, launches=launches)


@pytest.fixture(scope="module", params=["tiny_p2e", "tiny_p2e_ac"])
def fused_run(request):
    name = request.param
    run = _update(name, fused=True)
    run.update(g=_gold(name), exp=Hh.oracle_p2e_update(name))
    return run


def test_fused_ensemble_update(fused_run):
    g, exp, mets, p2e = fused_run["g"], fused_run["exp"], fused_run["mets"], fused_run["p2e"]
    for ref, src in ((torch.from_numpy(np.asarray(g["train/explorer_loss"])), "reference"), (exp["explorer_loss"], "oracle")):
        close(torch.tensor(mets["explorer_loss"]), ref, tol=1e-5, what=f"explorer_loss vs {src}")
    close(torch.tensor(mets["explorer_grad_norm"]), torch.from_numpy(np.asarray(g["train/explorer_grad_norm"])),
          tol=GTOL, what="explorer_grad_norm")
    n = 0
    for k, gr in fused_run["grads"].items():
        if k.startswith("_networks."):
            close(gr, torch.from_numpy(g["grad/" + k]), tol=GTOL, what="reference grad/" + k)
            close(gr, exp["explorer_grads"][k], tol=GTOL, what="oracle grad/" + k)
            n += 1
    assert n == len(exp["explorer_grads"])
    sd = p2e.state_dict()
    for k in exp["explorer_grads"]:
        adam_close(sd[k], torch.from_numpy(g["after/" + k]), 1e-4, "after/" + k)


def test_fused_behaviour_update(fused_run):
    name, g, exp, mets, p2e = fused_run["name"], fused_run["g"], fused_run["exp"], fused_run["mets"], fused_run["p2e"]
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    beh = p2e._behavior
    unperm = lambda x: Hh.from_time_major_rows(x, B, T)
    close(unperm(beh._last["reward"]), torch.from_numpy(g["imag/reward"]).squeeze(-1), what="intrinsic reward (reference)")
    close(unperm(beh._last["reward"]), exp["beh"]["reward"].squeeze(-1), what="intrinsic reward (oracle)")
    close(unperm(beh._last["target"]), exp["beh"]["target"].squeeze(-1), what="lambda-return")
    for k in ("actor_loss", "value_loss", "EMA_005", "EMA_095", "actor_entropy", "imag_reward_mean", "target_mean"):
        close(torch.tensor(mets[k]), torch.from_numpy(np.asarray(g["train/" + k])), tol=2e-5, what=k)
    close(torch.tensor(mets["actor_grad_norm"]), torch.from_numpy(np.asarray(g["train/actor_grad_norm"])),
          tol=GTOL, what="actor_grad_norm")
    close(torch.tensor(mets["value_grad_norm"]), torch.from_numpy(np.asarray(g["train/value_grad_norm"])),
          tol=GTOL, what="value_grad_norm")
    n = 0
    for k, gr in fused_run["grads"].items():
        if k.startswith(("_behavior.actor.", "_behavior.value.")):
            close(gr, torch.from_numpy(g["grad/" + k]), tol=GTOL, what="reference grad/" + k)
            n += 1
    assert n == len(exp["actor_grads"]) + len(exp["value_grads"])
    sd = p2e.state_dict()
    for k in sd:
        if k.startswith(("_behavior.actor.", "_behavior.value.")):
            adam_close(sd[k], torch.from_numpy(g["after/" + k]), 3e-5, "after/" + k)
        elif k.startswith("_behavior._slow_value."):
            close(sd[k], torch.from_numpy(g["after/" + k]), tol=1e-6, what="after/" + k)
    # the ensemble objective was never probed or evaluated as a foreign (autograd) objective
    assert not beh.__dict__.get("_objective_kinds")


@pytest.mark.parametrize("name", ["tiny_p2e", "tiny_p2e_ac", "tiny_p2e_onehot"])
def test_fused_agrees_with_the_autograd_route(name):
    """The same update by `train` (expl_fused False) and fused, from identical weights.  tiny_p2e_onehot: the one-hot
    actor under imag_gradient "reinforce" -- no gradient flows through the reward, so no disagreement backward runs.
    (Nor does one without disag_action_cond: the objective sees the detached feat, as in the reference, so the reward
    reaches the dynamics through the action alone.)"""
    a, f = _update(name, fused=False), _update(name, fused=True, profile=True)
    assert set(a["mets"]) == set(f["mets"]), set(a["mets"]) ^ set(f["mets"])
    for k, v in a["mets"].items():
        close(torch.tensor(f["mets"][k]), torch.tensor(v), tol=1e-5, what=k)
    assert set(a["grads"]) == set(f["grads"])
    for k, v in a["grads"].items():
        close(f["grads"][k], v, tol=GTOL, what="grad " + k)
    bwd = [k for k in f["launches"] if "disag_bwd" in k]
    sh = common.SHAPES[name]
    if sh["imag_gradient"] == "reinforce" or not sh["p2e"]["disag_action_cond"]:
        assert not bwd and any("ens_disag_fwd_kernel" in k and "+mu" not in k for k in f["launches"]), list(f["launches"])
    else:
        assert bwd, list(f["launches"])


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


def test_agent_replays_the_fused_explorer():
    """dreamer.Dreamer with expl_behavior plan2explore: the runner captures the explorer half after its warm-up of 2 and
    replays it; an agent at hip_graph=False fed the same batches (eager launches) reaches the same explorer losses."""
    name = "tiny_p2e"
    seqs, agents = {}, {}
    for graph in (True, False):
        agent = _agent(name, hip_graph=graph)
        if not graph:
            agent.load_state_dict(start)
        else:
            start = {k: v.clone() for k, v in agent.state_dict().items()}
        for i in range(5):
            agent._train(common.make_batch(name, seed=i))
            agent._flush_metrics()  # (one entry per update in every metric's list)
        seqs[graph], agents[graph] = dict(agent._metrics), agent
    ga = agents[True]
    r = ga._runner
    assert r.use_graph and r.expl is ga._expl_behavior and r._g_expl is not None and len(r._g_expl) == 3
    assert agents[False]._runner._g_expl is None
    keys = {k for k in seqs[True] if k.startswith("expl_")}
    for k in ("expl_explorer_loss", "expl_explorer_grad_norm", "expl_actor_loss", "expl_value_loss", "expl_imag_reward_mean",
              "expl_actor_grad_norm", "expl_value_grad_norm", "expl_actor_entropy"):
        assert k in keys, (k, sorted(keys))
    assert keys == {k for k in seqs[False] if k.startswith("expl_")}
    for k in keys:
        assert len(seqs[True][k]) == 5 and np.all(np.isfinite(seqs[True][k])), (k, seqs[True][k])
    close(torch.tensor(seqs[True]["expl_explorer_loss"]), torch.tensor(seqs[False]["expl_explorer_loss"]), tol=1e-5,
          what="explorer loss over 5 updates, replay vs eager")
    # acting: the exploration actor while training
    obs = {k: v[:, 0] for k, v in common.make_batch(name).items()}
    obs = {k: obs[k] for k in ("image", "is_first", "is_terminal")}
    out_t, _ = ga._policy(obs, None, training=True)
    assert ga._exploring() and torch.isfinite(out_t["logprob"]).all()


def test_state_dict_round_trip_with_the_member_major_bucket():
    """The member-major explorer bucket renames nothing: same keys as with expl_fused off (the flat bucket), a round
    trip into a fresh agent, and the stacked views are the modules' own parameters."""
    name = "tiny_p2e"
    agent = _agent(name)
    agent._train(common.make_batch(name))
    sd = agent.state_dict()
    assert list(sd.keys()) == list(_agent(name, expl_fused=False).state_dict().keys())
    assert any(k.startswith("_expl_behavior._networks.2.layers.NoName_linear1.weight") for k in sd)
    fresh = _agent(name, seed=1)
    fresh.load_state_dict(sd)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k
    b = fresh._expl_behavior._expl_opt.bucket.ensure()
    assert b.members == common.SHAPES[name]["p2e"]["disag_models"]
    W0, _ = b.stacked(0)
    for i, net in enumerate(fresh._expl_behavior._networks):
        p = next(net.parameters())
        assert W0[i].data_ptr() == p.data_ptr() and torch.equal(W0[i], p)
