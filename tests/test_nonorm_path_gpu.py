"""Layers without LayerNorm (config keys norm / encoder.norm / decoder.norm: False) through the public classes against
the REFERENCE's own vectors (tests/golden/tiny_nonorm.npz, tiny_nonorm_mix.npz and tiny_nonorm_video.npz, written by
tests/golden/make_golden_nonorm.py): the world-model update, the behaviour update, a second consecutive update, the
behaviour on identical weights, the acting steps, the video slice, and hipGraph replay / the pipelined schedule against
eager launches.  The pattern, helpers and bars are those of tests/test_act_path_gpu.py.

  tiny_nonorm      the `tiny` row with all three keys False: categorical latents (the one-hot gathers stay on, followed
                   by the activation), continuous actor, imag_gradient dynamics
  tiny_nonorm_mix  norm False, encoder.norm True, decoder.norm False (a cross-wired key shows): dyn_discrete 0 (the
                   dense call sites), image + vector observations, one-hot actor (the second actor-head route), reinforce

Bars, imported from tests/gauss_helpers.py: outputs, states and metrics 1e-4 (losses of the first update 1e-5),
gradients against the reference's CPU vectors G.grad_tol (5e-6 of the tensor's max for the actor's and the critic's
tensors, GRAD_BOUND for the world model's), Adam-updated parameters 1e-6 (adam_close); replay and the pipelined
schedule at the bars of tests/test_pipeline_gpu.py for `tiny`.  Every draw is injected; the categorical ones are also
teacher-forced to the reference's classes, and the flip counter must stay at zero."""
import functools

import numpy as np
import pytest
import torch

from tests import nonorm_helpers as A
from tests import gauss_helpers as G
from tests import helpers as Hh
from tests.golden import nonorm_common as AC
from tests.golden import common

pytestmark = pytest.mark.gpu
NAMES = list(AC.NAMES)


def _dev(d):
    return {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in d.items()}


def _same_stoch(name, got, ref, what):
    if AC.gauss(name):
        G.close(got, ref, what=what)
    else:
        assert np.array_equal(got.detach().cpu().numpy(), np.asarray(ref)), f"{what}: sampled classes differ"


@functools.lru_cache(maxsize=None)
def _updates(name):
    """Two consecutive updates (world model, then the task behaviour)."""
    g = A.gold(name)
    cfg, wm, beh = A.build_models(name)
    flips = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = dict(name=name, cfg=cfg, wm=wm, beh=beh, g=g, updates=[])
    params_now = lambda: {**{k: v.clone() for k, v in wm.state_dict().items()},
                          **{k: v.clone() for k, v in beh.state_dict().items() if not k.startswith("_world_model.")}}
    for i, tr in enumerate(("train/", "train2/")):
        wm_noise, im_noise = A.gpu_noise(name, seed=i, g=g, tr=tr, flips=flips, prior=i == 0)
        data = AC.make_batch(name, seed=i)
        post, context, mets = wm._train(data, noise=wm_noise)
        u = dict(mets={k: float(v) for k, v in mets.items()},
                 wm_grads={k: p.grad.clone() for k, p in wm.named_parameters()},
                 post={k: v.clone() for k, v in post.items()})
        _, imag_state, action, weights, bmets = beh._train(u["post"], None, noise=im_noise)
        torch.cuda.synchronize()
        u.update(bmets={k: float(v) for k, v in bmets.items()}, after=params_now(),
                 imag_stoch=imag_state["stoch"].clone(), imag_action=action.clone())
        rec["updates"].append(u)
    rec["flips"] = int(flips.item())
    return rec


@pytest.fixture(scope="module", params=NAMES)
def act_run(request):
    return _updates(request.param)


def test_config_carries_the_norm_keys():
    ln = lambda m: any(isinstance(x, torch.nn.LayerNorm) for x in m.modules())
    for name in NAMES:
        s = common.SHAPES[name]
        cfg, wm, beh = A.build_models(name)
        assert (cfg.norm, cfg.encoder["norm"], cfg.decoder["norm"]) == (s["norm"], s["enc_norm"], s["dec_norm"])
        assert ln(wm.encoder) == s["enc_norm"] and ln(wm.heads["decoder"]) == s["dec_norm"]
        for m in (wm.dynamics, wm.heads["reward"], wm.heads["cont"], beh.actor, beh.value, beh._slow_value):
            assert ln(m) == s["norm"], type(m).__name__
        # g is None exactly where the LayerNorm is gone, and the engines keep no statistics for those layers
        P = wm.dynamics.params()
        assert all((L.g is None) == (not s["norm"]) for L in (P.img_in, P.gru, P.img_out, P.obs_out))
        assert all((L.g is None) == (not s["norm"]) for L in beh.actor.trunk_params())
    assert float(A.gold("tiny_nonorm")["meta/gru_pre_absmax"]) <= AC.GRU_PRE_MAX


@pytest.mark.parametrize("name", NAMES)
def test_fixture_holds_the_keys_the_path_test_reads(name):
    path = A.os.path.join(A.GOLDEN, name + ".npz")
    assert A.os.path.getsize(path) < (1 << 20)
    have = set(A.gold(name).files)
    missing = [k for k in A.fixture_keys(name) if k not in have]
    assert not missing, missing[:10]


def test_no_teacher_forced_draw_flipped(act_run):
    assert act_run["flips"] == 0, f"{act_run['flips']} categorical draws differ from the reference's"


def test_world_model_update(act_run):
    name, g = act_run["name"], act_run["g"]
    u = act_run["updates"][0]
    for k in AC.state_keys(name):
        if k == "stoch":
            _same_stoch(name, u["post"][k], g["post/stoch"], "post/stoch")
        else:
            G.close(u["post"][k], g["post/" + k], what="post/" + k)
    m = u["mets"]
    G.close(torch.tensor(m["model_loss"]), g["train/model_loss"], tol=1e-5, what="model_loss")
    for k in A.WM_METRICS + tuple(k + "_loss" for k in A.decoder_keys(name)):
        # (the reference logs dyn_loss / rep_loss per step, the fused path their mean)
        G.close(torch.tensor(m[k]), np.asarray(g["train/" + k]).mean(), what="train/" + k)
    G.close(torch.tensor(m["model_grad_norm"]), g["model_grad_norm"], tol=2e-5, what="model_grad_norm (float64 of the reference)")
    n = 0
    for k, gr in u["wm_grads"].items():
        G.grad_close(gr, g["grad/" + k], what="grad/" + k, tol=G.grad_tol(k))
        n += 1
    assert n == sum(1 for k in g.files if k.startswith("grad/") and k.split("/")[1].split(".")[0] in Hh.WM_PREFIXES)


def test_updates_parameters_and_metrics(act_run):
    """Post-Adam parameters and the reference's _train metrics after update 1 and after update 2 (Adam state, the slow
    critic and the return EMA carried across), and the imagined draws of both."""
    name, g = act_run["name"], act_run["g"]
    s = common.SHAPES[name]
    unperm = lambda x: Hh.from_time_major_rows(x, s["B"], s["T"])
    for i, (tr, af) in enumerate((("train/", "after/"), ("train2/", "after2/"))):
        u = act_run["updates"][i]
        m = {**u["mets"], **u["bmets"]}
        _same_stoch(name, u["post"]["stoch"], g[tr + "post/stoch"], tr + "post/stoch")
        G.close(u["post"]["deter"], g[tr + "post/deter"], what=tr + "post/deter")
        _same_stoch(name, unperm(u["imag_stoch"]), g[tr + "imag/stoch"], tr + "imag/stoch")
        G.close(unperm(u["imag_action"]), g[tr + "imag/action"], what=tr + "imag/action")
        for k in ("model_loss", "kl", "prior_ent", "post_ent") + A.BEH_METRICS:
            tol = (1e-5 if i == 0 else 5e-4) if k.endswith("_loss") else G.TOL
            G.close(torch.tensor(m[k]), g[tr + k], tol=tol, what=tr + k)
        for k in A.NORMS:
            G.close(torch.tensor(m[k]), g[tr + k], tol=G.TOL, what=tr + k)
        for k, v in u["after"].items():
            if k == "ema_vals":
                G.close(v, torch.tensor([float(g[tr + "EMA_005"]), float(g[tr + "EMA_095"])]), what=af + k)
            elif k.startswith("_slow_value.") and i == 0:
                G.close(v, g[af + k], tol=1e-6, what=af + k)
            else:
                lr = 1e-4 if k.split(".")[0] in Hh.WM_PREFIXES else 3e-5
                G.adam_close(v, g[af + k], lr, what=af + k, steps=i + 1)


@pytest.mark.parametrize("name", NAMES)
def test_behaviour_on_identical_weights(name):
    """World-model forward/backward WITHOUT its optimizer step, then the behaviour's losses and gradients on those
    weights: the setting of the fixture's imag/* and grad/actor.*, grad/value.* entries."""
    g = A.gold(name)
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    cfg, wm, beh = A.build_models(name)
    flips = torch.zeros(1, dtype=torch.int32, device="cuda")
    wm_noise, im_noise = A.gpu_noise(name, g=g, tr="", flips=flips)
    wm.train_fwd_bwd(AC.make_batch(name), noise=wm_noise)
    post = {k: v.clone() for k, v in wm._pending[0].items()}
    beh._update_slow_target = lambda: None
    beh.train_fwd_bwd(post, noise=im_noise)
    (_, imag_state, action, weights), _, (aloss, vloss) = beh._pending
    torch.cuda.synchronize()
    assert int(flips.item()) == 0
    unperm = lambda x: Hh.from_time_major_rows(x, B, T)
    assert {"stoch", "deter"} <= set(imag_state) <= set(AC.state_keys(name))
    for k in imag_state:
        if k == "stoch":
            _same_stoch(name, unperm(imag_state[k]), g["imag/stoch"], "imag/stoch")
        elif k != "logit":  # (step 0 of the reference's imagined logits is the start state's posterior logit)
            G.close(unperm(imag_state[k]), g["imag/" + k], what="imag/" + k)
    G.close(unperm(action), g["imag/action"], what="imag/action")
    feat = torch.cat([imag_state["stoch"].reshape(imag_state["stoch"].shape[:2] + (-1,)), imag_state["deter"]], -1)
    G.close(unperm(feat), g["imag/feat"], what="imag/feat")
    G.close(unperm(weights), g["imag/weights"], what="imag/weights")
    G.close(unperm(beh._last["reward"]), g["imag/reward"][..., 0], what="imag/reward")
    G.close(unperm(beh._last["target"]), g["imag/target"][..., 0], what="imag/target")
    G.close(unperm(beh._last["value"]), g["imag/value"][..., 0], what="imag/value")
    G.close(unperm(beh._im["ent"]), g["imag/actor_ent"], what="imag/actor_ent")
    G.close(aloss, g["actor_loss"], tol=1e-5, what="actor_loss")
    G.close(vloss, g["value_loss"], tol=1e-5, what="value_loss")
    G.close(beh.ema_vals, g["ema_vals_after"], what="ema_vals")
    params = dict(beh.named_parameters())
    n = 0
    for key in g.files:
        if key.startswith("grad/actor.") or key.startswith("grad/value."):
            k = key[len("grad/"):]
            G.grad_close(params[k].grad, g[key], what=key, tol=G.grad_tol(k))
            n += 1
    assert n == sum(1 for k in AC.param_shapes(name) if k.startswith(("actor.", "value."))) >= 8


def test_video_pred_matches_the_reference():
    name = AC.VIDEO
    g = np.load(A.os.path.join(A.GOLDEN, name + "_video.npz"), allow_pickle=False)
    _, wm, _ = A.build_models(name)
    noise = _dev(AC.src(name).make_video_noise(name))
    video = wm.video_pred(AC.make_batch(name), noise=noise).cpu().numpy()
    assert tuple(video.shape) == tuple(g["meta/shape"])
    err = np.abs(video[:, :, 64:128] - g["video_model"]).max()
    print(f"[video] max err {err:.3e}")
    assert err <= 1e-4
    ref, got = g["sum/video"], common.checksum(video)
    assert abs(got[0] - ref[0]) <= 1e-4 * ref[1] and abs(got[1] - ref[1]) <= 1e-4 * ref[1]


# ---------------------------------------------------------------------------------------------
# hipGraph replay and the pipelined schedule against eager serial launches
# ---------------------------------------------------------------------------------------------
def _run(name, n_calls, mode):
    """mode: "eager" (every update launched eagerly), "graph" (call 0 eager, then hipGraph replay), "pipe"
    (step_pipelined + flush).  Learning rates 0: the exact claim."""
    import tools
    from dv3hip import shapes
    from dv3hip.graph import UpdateRunner

    cfg, wm, beh = A.build_models(name)
    for opt in (wm._model_opt, beh._actor_opt, beh._value_opt):
        opt._opt.param_groups[0]["lr"] = 0.0
    tools.default_rng("cuda:0", seed=7)
    r = UpdateRunner(wm, beh, use_graph=mode != "eager", warm=1)
    data = [{k: torch.from_numpy(v).cuda() for k, v in shapes.synthetic_batch(name, seed).items()} for seed in range(n_calls)]
    rec = dict(post=[], post_deter=[], im_stoch=[], im_action=[], g_model=[], g_actor=[], g_value=[], model_loss=[],
               actor_loss=[], value_loss=[], expl_loss=[])

    def grab_wm():
        torch.cuda.synchronize()
        rec["post"].append(r.last_post["stoch"].clone())
        rec["post_deter"].append(r.last_post["deter"].clone())
        rec["g_model"].append(wm._model_opt.bucket.grad.clone())
        rec["model_loss"].append(float(r.last_metrics["model_loss"]))

    def grab_beh():
        torch.cuda.synchronize()
        rec["im_stoch"].append(beh._im["stoch"].clone())
        rec["im_action"].append(beh._im["action"].clone())
        rec["g_actor"].append(beh._actor_opt.bucket.grad.clone())
        rec["g_value"].append(beh._value_opt.bucket.grad.clone())
        rec["actor_loss"].append(float(r.last_metrics["actor_loss"]))
        rec["value_loss"].append(float(r.last_metrics["value_loss"]))

    for d in data:
        if mode != "pipe":
            r.step(d, eager=mode == "eager")
            grab_wm(), grab_beh()
            continue
        pending = r._pipe_pending
        r.step_pipelined(d)
        if pending:
            grab_beh()
        grab_wm()
        if not r._pipe_pending:
            grab_beh()
    if mode == "pipe":
        was = r._pipe_pending
        r.flush()
        if was:
            grab_beh()
    if mode != "eager":
        assert r.use_graph, "hipGraph capture was refused"
    torch.cuda.synchronize()
    rec["pipe"] = r._pipe is not None
    rec["params"] = {k: v.detach().clone() for k, v in list(wm.state_dict().items()) + list(beh.state_dict().items())}
    rec["ema"] = beh.ema_vals.clone()
    rec["rng"] = tools.default_rng("cuda:0").state.clone()
    r.close()
    return rec


def _same_run(a, b, n):
    """tests/test_gauss_path_gpu.py::_same_run for either latent kind."""
    assert torch.equal(a["rng"], b["rng"]), "the Philox stream ends elsewhere"
    for key in ("post", "post_deter", "im_stoch", "im_action"):
        assert len(a[key]) == len(b[key]) == n, (key, len(a[key]), len(b[key]))
        for i in range(n):
            assert torch.equal(a[key][i], b[key][i]), f"update {i}: {key} differs"
    for key in ("g_model", "g_actor", "g_value"):
        for i in range(n):
            scale = float(a[key][i].abs().max())
            err = float((a[key][i] - b[key][i]).abs().max())
            print(f"[replay] update {i} {key}: err {err:.3e} max {scale:.3e}")
            assert err <= 4e-6 * scale + 1e-12, f"update {i}: {key} differs by {err:.3e} (max |g| {scale:.3e})"
    for key in ("model_loss", "actor_loss", "value_loss", "expl_loss"):
        assert len(a[key]) == len(b[key])
        np.testing.assert_allclose(b[key], a[key], rtol=2e-6, atol=1e-6, err_msg=key)
    assert torch.allclose(a["ema"], b["ema"], rtol=1e-6, atol=1e-7), (a["ema"], b["ema"])
    for k, v in a["params"].items():  # (learning rates 0: nothing moves but the slow critic, by the same EMA steps)
        assert torch.equal(v, b["params"][k]), k


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_equals_eager(name):
    """Every update's sampled states and actions bit-equal between eager launches and hipGraph replay (use_graph still
    true after the warm-up), gradients equal up to the atomic summation order of the reverse scan."""
    n = 4
    _same_run(_run(name, n, "eager"), _run(name, n, "graph"), n)


def test_pipelined_updates_equal_serial_updates():
    """step_pipelined + flush at tiny_nonorm against the serial replay."""
    n = 5
    a, b = _run("tiny_nonorm", n, "graph"), _run("tiny_nonorm", n, "pipe")
    _same_run(a, b, n)


# ---------------------------------------------------------------------------------------------
# acting
# ---------------------------------------------------------------------------------------------
class _Logger:
    def __init__(self):
        self.step = 0

    def scalar(self, k, v):
        pass

    def video(self, *a, **k):
        pass

    def write(self, fps=False):
        pass


def _agent(name, eval_state_mean):
    import dreamer

    cfg = Hh.make_config(name)
    cfg.pretrain = 0
    cfg.eval_state_mean = eval_state_mean
    cfg.expl_behavior = "greedy"  # (the fixture's acting steps use the task actor)

    def dataset():
        while True:
            yield AC.make_batch(name)

    agent = dreamer.Dreamer(Hh.obs_space(name), None, cfg, _Logger(), dataset()).to(cfg.device)
    w = AC.make_weights(name)
    sd = agent.state_dict()
    for k in sd:
        key = k.replace("_wm.", "", 1) if k.startswith("_wm.") else k.replace("_task_behavior.", "", 1)
        if key.startswith("_world_model."):
            key = key[len("_world_model."):]
        if key in w:
            sd[k] = torch.from_numpy(w[key])
    agent.load_state_dict(sd)
    agent.requires_grad_(False)
    return agent


@pytest.mark.parametrize("name,tag", [(n, "train") for n in NAMES] + [("tiny_nonorm_mix", "eval")])
def test_policy_steps_match_the_reference(name, tag):
    """Three consecutive acting steps on two environments through Dreamer._policy (all reset at step 0, one env reset
    at step 1): sampled while training; for continuous latents also with eval_state_mean (stoch = mean, actor's mode)."""
    g = A.gold(name)
    training = tag == "train"
    agent = _agent(name, eval_state_mean=not training)
    state = None
    for t, st in enumerate(AC.make_policy_inputs(name)):
        obs = {k: st[k] for k in AC.obs_keys(name)}
        noise = _dev({k: st[k] for k in ("prior", "post", "act")})
        out, state = agent._policy(obs, state, training, noise=noise)
        latent, action = state
        pre = f"policy/{tag}/{t}/"
        assert set(latent) == set(AC.state_keys(name))
        for k in AC.state_keys(name):
            if k == "stoch":
                _same_stoch(name, latent[k], g[pre + k], pre + k)
            else:
                G.close(latent[k], g[pre + k], what=pre + k)
        G.close(out["action"], g[pre + "action"], what=pre + "action")
        G.close(out["logprob"], g[pre + "logprob"], tol=2e-4, what=pre + "logprob")


@pytest.mark.parametrize("name", NAMES)
def test_policy_graph_replay_equals_eager(name):
    """graph.PolicyRunner replays the acting step of a LayerNorm-free model: the same states and actions as eager launches."""
    import tools

    agent = _agent(name, False)
    steps = AC.make_policy_inputs(name) + AC.make_policy_inputs(name, seed=1)[1:]
    outs = {}
    for mode in ("eager", "graph"):
        tools.default_rng(agent._config.device, seed=21)
        state, res = None, []
        for t, st in enumerate(steps):
            obs = {k: st[k] for k in AC.obs_keys(name)}
            training = t != len(steps) - 1
            if mode == "eager":
                out, state = agent._policy_eager(obs, state, training)
            else:
                out, state = agent._policy(obs, state, training)
            res.append((out["action"].clone(), out["logprob"].clone(), {k: v.clone() for k, v in state[0].items()}))
        outs[mode] = res
    assert agent._policy_runner not in (None, False) and len(agent._policy_runner._sig) == 2
    for (a0, l0, s0), (a1, l1, s1) in zip(outs["eager"], outs["graph"]):
        assert set(s0) == set(s1) == set(AC.state_keys(name))
        for k in s0:
            assert torch.allclose(s0[k], s1[k], atol=1e-6), k
        assert torch.allclose(a0, a1, atol=1e-6) and torch.allclose(l0, l1, atol=1e-5)
