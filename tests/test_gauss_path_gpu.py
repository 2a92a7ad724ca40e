"""Continuous Gaussian latents (dyn_discrete: 0) on the MI355X path against the REFERENCE's own vectors
(tests/golden/tiny_gauss*.npz, cfg2_gauss.npz, written by tests/golden/make_golden_gauss.py): the public classes
forward, the autograd surface, the fused update (WorldModel._train + ImagBehavior._train, two consecutive updates),
hipGraph replay and the pipelined schedule against eager serial launches, and the acting step.

Every draw is injected (N(0,1) tapes), the sample is continuous: nothing is teacher-forced and there are no flips to
count.  Bars (tests/gauss_helpers.py, with the measurements behind the gradient bound): outputs and states 1e-4,
gradients 6.4e-5 of the tensor's max (twice the discrete shapes' measured worst against their reference vectors; most
tensors meet 5e-6), Adam-updated parameters 1e-6 up to the sign-like first steps of near-zero gradients."""
import numpy as np
import pytest
import torch

from tests import gauss_helpers as G
from tests import helpers as Hh
from tests.golden import common, gauss_common as GC

pytestmark = pytest.mark.gpu

TINY = ["tiny_gauss", "tiny_gauss_onehot"]
ALL = TINY + ["cfg2_gauss"]
STATE_KEYS = ("stoch", "deter", "mean", "std")


def _dev(d):
    return {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------
# public classes, forward only
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_public_forward(name):
    g = G.gold(name)
    full = bool(g["meta/full"])
    sel = slice(0, 2) if full else slice(0, 1)
    cfg, wm, _ = G.build_models(name)
    wm_noise, _ = G.gpu_noise(name)
    data = GC.make_batch(name)
    dyn = wm.dynamics
    with torch.no_grad():
        obs = wm.preprocess(data)
        embed = wm.encoder(obs)
        post, prior = dyn.observe(embed, obs["action"], obs["is_first"], noise=wm_noise)
        assert set(post) == set(STATE_KEYS) == set(prior)
        kl_loss, kl_value, dyn_loss, rep_loss = dyn.kl_loss(post, prior, cfg.kl_free, cfg.dyn_scale, cfg.rep_scale)
        feat = dyn.get_feat(post)
        assert feat.shape[-1] == cfg.dyn_stoch + cfg.dyn_deter
        preds = {}
        for hname, head in wm.heads.items():
            pred = head(feat)
            preds.update(pred if isinstance(pred, dict) else {hname: pred})
        losses = {k: -pred.log_prob(obs[k]) for k, pred in preds.items()}
        ent_post, ent_prior = dyn.get_dist(post).entropy(), dyn.get_dist(prior).entropy()
    G.close(embed if full else embed[sel, :8], g["embed"], what="embed")
    for k in STATE_KEYS:
        G.close(post[k] if full else post[k][sel], g["post/" + k], what="post/" + k)
        # (prior deter IS post deter, networks.py:205: the full-size fixture stores it once)
        G.close(prior[k] if full else prior[k][sel], g[("post/" if k == "deter" and not full else "prior/") + k],
                what="prior/" + k)
        G.checksum_close(g, "post/" + k, post[k])
    G.close(kl_value, g["kl_value"], what="kl_value")
    G.close(kl_loss, g["kl_loss"], what="kl_loss")
    G.close(dyn_loss, g["dyn_loss"], what="dyn_loss")
    G.close(rep_loss, g["rep_loss"], what="rep_loss")
    # both sides of the free-bits clip are on the table
    assert (g["kl_value"] < cfg.kl_free).any() and (g["kl_value"] > cfg.kl_free).any()
    G.close(ent_post, g["post_ent"], what="post_ent")
    G.close(ent_prior, g["prior_ent"], what="prior_ent")
    G.close(preds["image"].mode()[0:1, 0:2], g["recon"], what="recon")
    G.checksum_close(g, "recon", preds["image"].mode())
    for k, v in losses.items():
        G.close(v, g["loss/" + k], what="loss/" + k)
    # the mode / the sample of the latent distribution object
    dist = dyn.get_dist(post)
    assert torch.equal(dist.mode(), post["mean"]) and dist.mean is post["mean"] and dist.stddev is post["std"]
    eps = wm_noise["q_post"].transpose(0, 1).contiguous()
    smp = dist.sample(noise=eps)
    G.close(smp if full else smp[sel], g["post/stoch"], what="get_dist().sample")


@pytest.mark.parametrize("name", TINY)
def test_obs_step_img_step_and_carried_state(name):
    """obs_step called step by step, observe with a carried state, img_step and imagine_with_action give what the one
    scan gives (and the fixture holds)."""
    g = G.gold(name)
    cfg, wm, _ = G.build_models(name)
    wm_noise, _ = G.gpu_noise(name)
    data = GC.make_batch(name)
    dyn = wm.dynamics
    s = common.SHAPES[name]
    T = s["T"]
    with torch.no_grad():
        obs = wm.preprocess(data)
        embed = wm.encoder(obs)
        state, action = None, None
        posts, priors = [], []
        for t in range(T):
            nz = dict(prior=wm_noise["q_prior"][t], post=wm_noise["q_post"][t])
            post, prior = dyn.obs_step(state, obs["action"][:, t] if state is not None else None, embed[:, t],
                                       obs["is_first"][:, t], noise=nz)
            posts.append(post), priors.append(prior)
            state = post
        for k in STATE_KEYS:
            G.close(torch.stack([p[k] for p in posts], 1), g["post/" + k], what="obs_step post/" + k)
            G.close(torch.stack([p[k] for p in priors], 1), g["prior/" + k], what="obs_step prior/" + k)
        # observe in two halves, the second one from the carried state
        h = T // 2
        nz1 = {k: v[:h].contiguous() for k, v in wm_noise.items()}
        nz2 = {k: v[h:].contiguous() for k, v in wm_noise.items()}
        p1, _ = dyn.observe(embed[:, :h], obs["action"][:, :h], obs["is_first"][:, :h], noise=nz1)
        last = {k: v[:, -1] for k, v in p1.items()}
        p2, q2 = dyn.observe(embed[:, h:], obs["action"][:, h:], obs["is_first"][:, h:], state=last, noise=nz2)
        for k in STATE_KEYS:
            G.close(torch.cat([p1[k], p2[k]], 1), g["post/" + k], what="carried observe post/" + k)
            G.close(q2[k], g["prior/" + k][:, h:], what="carried observe prior/" + k)
        # img_step from the posterior of step t with the action of step t+1 is the prior of step t+1 where no reset falls
        first = obs["is_first"].bool()
        t = next(t for t in range(T - 1) if not first[:, t + 1].any())
        st = {k: torch.from_numpy(g["post/" + k][:, t]).cuda() for k in STATE_KEYS}
        pri = dyn.img_step(st, obs["action"][:, t + 1], noise=wm_noise["q_prior"][t + 1])
        for k in STATE_KEYS:
            G.close(pri[k], g["prior/" + k][:, t + 1], what="img_step " + k)
        pri_mode = dyn.img_step(st, obs["action"][:, t + 1], sample=False)
        assert torch.equal(pri_mode["stoch"], pri_mode["mean"])
        roll = dyn.imagine_with_action(obs["action"][:, t + 1:t + 2], st, noise=wm_noise["q_prior"][t + 1:t + 2])
        for k in STATE_KEYS:
            G.close(roll[k][:, 0], g["prior/" + k][:, t + 1], what="imagine_with_action " + k)
        init = dyn.initial(3)
        assert set(init) == set(STATE_KEYS) and float(init["mean"].abs().max()) == 0.0
        G.close(init["stoch"], dyn.get_stoch(init["deter"]), tol=1e-6, what="initial stoch = get_stoch(tanh(W))")


def test_latent_entropy_is_differentiable():
    """get_dist(state).entropy() in a loss: value and gradient of torch.distributions' Normal in float64."""
    import torch.distributions as torchd

    _, wm, _ = G.build_models("tiny_gauss")
    gen = torch.Generator().manual_seed(3)
    mean, std = torch.randn(5, 7, 8, generator=gen), 0.1 + torch.rand(5, 7, 8, generator=gen)
    up = torch.randn(5, 7, generator=gen)
    m64, s64 = mean.double().requires_grad_(True), std.double().requires_grad_(True)
    ent_ref = torchd.Independent(torchd.Normal(m64, s64), 1).entropy()
    (ent_ref * up.double()).sum().backward()
    mg, sg = mean.cuda().requires_grad_(True), std.cuda().requires_grad_(True)
    ent = wm.dynamics.get_dist({"mean": mg, "std": sg}).entropy()
    (ent * up.cuda()).sum().backward()
    G.close(ent, ent_ref, what="entropy")
    G.grad_close(sg.grad, s64.grad, what="d entropy / d std", tol=G.GRAD_TOL)
    assert mg.grad is None or float(mg.grad.abs().max()) == 0.0


def test_video_pred_matches_the_reference():
    name = "tiny_gauss"
    g = np.load(G.os.path.join(G.GOLDEN, name + "_video.npz"), allow_pickle=False)
    _, wm, _ = G.build_models(name)
    noise = _dev(GC.make_video_noise(name))
    video = wm.video_pred(GC.make_batch(name), noise=noise).cpu().numpy()
    assert tuple(video.shape) == tuple(g["meta/shape"])
    err = np.abs(video[:, :, 64:128] - g["video_model"]).max()
    print(f"[video] max err {err:.3e}")
    assert err <= 1e-4
    ref, got = g["sum/video"], common.checksum(video)
    assert abs(got[0] - ref[0]) <= 1e-4 * ref[1] and abs(got[1] - ref[1]) <= 1e-4 * ref[1]


# ---------------------------------------------------------------------------------------------
# autograd surface
# ---------------------------------------------------------------------------------------------
def _public_loss(wm, cfg, data, wm_noise, stepwise):
    obs = wm.preprocess(data)
    embed = wm.encoder(obs)
    dyn = wm.dynamics
    if stepwise:  # obs_step's chain of autograd nodes instead of the one ObserveFn node
        state, posts, priors = None, [], []
        for t in range(embed.shape[1]):
            nz = dict(prior=wm_noise["q_prior"][t], post=wm_noise["q_post"][t])
            post, prior = dyn.obs_step(state, obs["action"][:, t] if state is not None else None, embed[:, t],
                                       obs["is_first"][:, t], noise=nz)
            posts.append(post), priors.append(prior)
            state = post
        post = {k: torch.stack([p[k] for p in posts], 1) for k in STATE_KEYS}
        prior = {k: torch.stack([p[k] for p in priors], 1) for k in STATE_KEYS}
    else:
        post, prior = dyn.observe(embed, obs["action"], obs["is_first"], noise=wm_noise)
    kl_loss, kl_value, _, _ = dyn.kl_loss(post, prior, cfg.kl_free, cfg.dyn_scale, cfg.rep_scale)
    feat = dyn.get_feat(post)
    preds = {}
    for hname, head in wm.heads.items():
        pred = head(feat)
        preds.update(pred if isinstance(pred, dict) else {hname: pred})
    losses = {k: -pred.log_prob(obs[k]) for k, pred in preds.items()}
    return torch.mean(sum(losses.values()) + kl_loss), post, kl_value


@pytest.mark.parametrize("stepwise", [False, True])
@pytest.mark.parametrize("name", TINY)
def test_autograd_surface_world_model_update(name, stepwise):
    """The reference's WorldModel._train written against the public methods with loss.backward(): the reference's
    gradients and post-Adam parameters."""
    import tools

    g = G.gold(name)
    cfg, wm, _ = G.build_models(name)
    wm_noise, _ = G.gpu_noise(name)
    with tools.RequiresGrad(wm):
        loss, post, kl_value = _public_loss(wm, cfg, GC.make_batch(name), wm_noise, stepwise)
        mets = wm._model_opt(loss, wm.parameters())
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        G.close(post[k], g["post/" + k], what="post/" + k)
    G.close(kl_value, g["kl_value"], what="kl_value")
    G.close(torch.tensor(float(mets["model_loss"])), g["model_loss"], tol=1e-5, what="model_loss")
    G.close(torch.tensor(float(mets["model_grad_norm"])), g["model_grad_norm"], tol=2e-5, what="model_grad_norm")
    for k, p in wm.named_parameters():
        G.grad_close(p.grad, g["grad/" + k], what="grad/" + k, tol=G.grad_tol(k))
    for k, v in wm.state_dict().items():
        G.adam_close(v, g["after/" + k], 1e-4, what="after/" + k)


# ---------------------------------------------------------------------------------------------
# the fused update: two consecutive updates against the reference's _train pair
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ALL)
def gauss_run(request):
    name = request.param
    cfg, wm, beh = G.build_models(name)
    rec = dict(name=name, cfg=cfg, wm=wm, beh=beh, updates=[])
    params_now = lambda: {**{k: v.clone() for k, v in wm.state_dict().items()},
                          **{k: v.clone() for k, v in beh.state_dict().items() if not k.startswith("_world_model.")}}
    for i in range(2):
        wm_noise, im_noise = G.gpu_noise(name, seed=i)
        before = params_now()
        post, context, mets = wm._train(GC.make_batch(name, seed=i), noise=wm_noise)
        u = dict(mets={k: float(v) for k, v in mets.items()},
                 wm_grads={k: p.grad.clone() for k, p in wm.named_parameters()},
                 post={k: v.clone() for k, v in post.items()})
        _, imag_state, action, weights, bmets = beh._train(u["post"], None, noise=im_noise)
        torch.cuda.synchronize()
        u.update(bmets={k: float(v) for k, v in bmets.items()}, before=before, after=params_now())
        rec["updates"].append(u)
    return rec


def _grad_check(g, name, k, grad):
    """A gradient against the fixture: element-wise where it holds the tensor; at full size the reference's (sum,
    abs-sum, max-abs) at 1e-4 of the abs-sum and the SAMPLE stored elements at the gradient bar, relative to the whole
    tensor's max."""
    if bool(g["meta/full"]):
        G.grad_close(grad, g["grad/" + k], what="grad/" + k, tol=G.grad_tol(k))
        return
    G.checksum_close(g, "grad/" + k, grad)
    got, ref = G.sampled(g, name, "grad", k, grad)
    G.grad_close(got, ref, what="smp/grad/" + k, tol=G.grad_tol(k), scale=float(g["sum/grad/" + k][2]))


# Relative tolerance of the delta checksums (after - before, per tensor) at full size: a step is lr-sized (Adam's first
# steps are lr g / (|g| + eps), |.| <= lr = 3e-5 for the actor and the critic, 1e-4 for the world model) and both sides
# store before + step in fp32, i.e. rounded to 6e-8 |w| with |w| up to ~1: 6e-8 / 3e-5 = 2e-3 of the step.
DELTA_TOL = 2e-3


def test_fused_world_model_update(gauss_run):
    name, g = gauss_run["name"], G.gold(gauss_run["name"])
    full = bool(g["meta/full"])
    sel = slice(0, 2) if full else slice(0, 1)
    u = gauss_run["updates"][0]
    for k in STATE_KEYS:
        G.close(u["post"][k] if full else u["post"][k][sel], g["post/" + k], what="post/" + k)
        G.checksum_close(g, "post/" + k, u["post"][k])
    m = u["mets"]
    G.close(torch.tensor(m["model_loss"]), g["train/model_loss"], tol=1e-5, what="model_loss")
    for k in ("kl", "prior_ent", "post_ent", "dyn_loss", "rep_loss", "image_loss", "reward_loss", "cont_loss"):
        # (the reference logs dyn_loss / rep_loss per step, the fused path their mean)
        G.close(torch.tensor(m[k]), np.asarray(g["train/" + k]).mean(), what="train/" + k)
    G.close(torch.tensor(m["model_grad_norm"]), g["model_grad_norm"], tol=2e-5, what="model_grad_norm (float64 of the reference)")
    n = 0
    for k, gr in u["wm_grads"].items():
        _grad_check(g, name, k, gr)
        n += 1
    assert n == sum(1 for k in g.files if k.startswith("sum/grad/") and k.split("/")[2].split(".")[0] in Hh.WM_PREFIXES)


def test_fused_updates_parameters_and_metrics(gauss_run):
    """Post-Adam parameters and the reference's _train metrics after update 1 and after update 2 (Adam state, the slow
    critic and the return EMA carried across)."""
    name, g = gauss_run["name"], G.gold(gauss_run["name"])
    full = bool(g["meta/full"])
    for i, (tr, af) in enumerate((("train/", "after/"), ("train2/", "after2/"))):
        u = gauss_run["updates"][i]
        m = {**u["mets"], **u["bmets"]}
        for k in ("model_loss", "kl", "prior_ent", "post_ent", "actor_loss", "value_loss", "actor_entropy", "EMA_005",
                  "EMA_095", "target_mean", "target_std", "imag_reward_mean", "value_mean"):
            tol = (1e-5 if i == 0 else 5e-4) if k.endswith("_loss") else G.TOL
            G.close(torch.tensor(m[k]), g[tr + k], tol=tol, what=tr + k)
        for k in ("model_grad_norm", "actor_grad_norm", "value_grad_norm"):
            G.close(torch.tensor(m[k]), g[tr + k], tol=G.TOL, what=tr + k)
        for k, v in u["after"].items():
            if k == "ema_vals":
                G.close(v, torch.tensor([float(g[tr + "EMA_005"]), float(g[tr + "EMA_095"])]), what=af + k)
            elif full and k.startswith("_slow_value.") and i == 0:
                G.close(v, g[af + k], tol=1e-6, what=af + k)
            elif full:
                lr = 1e-4 if k.split(".")[0] in Hh.WM_PREFIXES else 3e-5
                G.adam_close(v, g[af + k], lr, what=af + k, steps=i + 1)
            else:
                # full size: the stored elements at the Adam bar, and what the update did to the whole tensor
                # (after - before) against the reference's checksum of the same difference
                got, ref = G.sampled(g, name, af[:-1], k, v)
                if k.startswith("_slow_value.") and i == 0:
                    G.close(got, ref, tol=1e-6, what="smp/" + af + k)
                else:
                    lr = 1e-4 if k.split(".")[0] in Hh.WM_PREFIXES else 3e-5
                    G.adam_close(got, ref, lr, what="smp/" + af + k, steps=i + 1)
                row = GC.delta_names(name).index(k)
                delta = v.double() - u["before"][k].double()
                G.checksum_close(g, "delta/" + af + k, delta, tol=DELTA_TOL * (i + 1), ref=g["sum/delta/" + af[:-1]][row])


@pytest.mark.parametrize("name", ALL)
def test_behaviour_on_identical_weights(name):
    """World-model forward/backward WITHOUT its optimizer step, then the behaviour's losses and gradients on those
    weights: the setting of the fixture's imag/* and grad/actor.*, grad/value.* entries."""
    g = G.gold(name)
    full = bool(g["meta/full"])
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    nrow = 8 if full else 4
    cfg, wm, beh = G.build_models(name)
    wm_noise, im_noise = G.gpu_noise(name)
    wm.train_fwd_bwd(GC.make_batch(name), noise=wm_noise)
    post = {k: v.clone() for k, v in wm._pending[0].items()}
    beh._update_slow_target = lambda: None
    beh.train_fwd_bwd(post, noise=im_noise)
    (_, imag_state, action, weights), _, (aloss, vloss) = beh._pending
    torch.cuda.synchronize()
    unperm = lambda x: Hh.from_time_major_rows(x, B, T)
    part = (lambda x: x) if full else (lambda x: x[:, :nrow])
    assert set(imag_state) == set(STATE_KEYS)
    for k in ("stoch", "deter"):
        G.close(part(unperm(imag_state[k])), g["imag/" + k], what="imag/" + k)
    for k in ("mean", "std"):  # (step 0 is the start state's own posterior statistics)
        G.close(part(unperm(imag_state[k])), g["imag/" + k], what="imag/" + k)
    G.close(part(unperm(action)), g["imag/action"], what="imag/action")
    feat = torch.cat([imag_state["stoch"], imag_state["deter"]], -1)
    G.close(part(unperm(feat)), g["imag/feat"], what="imag/feat")
    G.close(part(unperm(weights)), g["imag/weights"], what="imag/weights")
    G.close(part(unperm(beh._last["reward"])), g["imag/reward"][..., 0], what="imag/reward")
    G.close(part(unperm(beh._last["target"])), g["imag/target"][..., 0], what="imag/target")
    G.close(part(unperm(beh._last["value"])), g["imag/value"][..., 0], what="imag/value")
    G.close(part(unperm(beh._im["ent"])), g["imag/actor_ent"], what="imag/actor_ent")
    G.close(aloss, g["actor_loss"], tol=1e-5, what="actor_loss")
    G.close(vloss, g["value_loss"], tol=1e-5, what="value_loss")
    G.close(beh.ema_vals, g["ema_vals_after"], what="ema_vals")
    params = dict(beh.named_parameters())
    for key in g.files:
        if key.startswith("sum/grad/actor.") or key.startswith("sum/grad/value."):
            k = key[len("sum/grad/"):]
            _grad_check(g, name, k, params[k].grad)


# ---------------------------------------------------------------------------------------------
# hipGraph replay and the pipelined schedule against eager serial launches
# ---------------------------------------------------------------------------------------------
def _run(name, n_calls, mode, lr_zero=True):
    """mode: "eager" (every update launched eagerly), "graph" (call 0 eager, then hipGraph replay), "pipe"
    (step_pipelined + flush)."""
    import tools
    from dv3hip import shapes
    from dv3hip.graph import UpdateRunner

    cfg, wm, beh = G.build_models(name)
    if lr_zero:
        for opt in (wm._model_opt, beh._actor_opt, beh._value_opt):
            opt._opt.param_groups[0]["lr"] = 0.0
    tools.default_rng("cuda:0", seed=7)
    r = UpdateRunner(wm, beh, use_graph=mode != "eager", warm=1)
    data = [{k: torch.from_numpy(v).cuda() for k, v in shapes.synthetic_batch(name, seed).items()} for seed in range(n_calls)]
    rec = dict(post=[], post_mean=[], im_stoch=[], im_action=[], g_model=[], g_actor=[], g_value=[], model_loss=[],
               actor_loss=[], value_loss=[])

    def grab_wm():
        torch.cuda.synchronize()
        rec["post"].append(r.last_post["stoch"].clone())
        rec["post_mean"].append(r.last_post["mean"].clone())
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
    assert torch.equal(a["rng"], b["rng"]), "the Philox stream ends elsewhere"
    for key in ("post", "post_mean", "im_stoch", "im_action"):
        assert len(a[key]) == len(b[key]) == n, (key, len(a[key]), len(b[key]))
        for i in range(n):
            assert torch.equal(a[key][i], b[key][i]), f"update {i}: {key} differs"
    for key in ("g_model", "g_actor", "g_value"):
        for i in range(n):
            scale = float(a[key][i].abs().max())
            err = float((a[key][i] - b[key][i]).abs().max())
            print(f"[replay] update {i} {key}: err {err:.3e} max {scale:.3e}")
            assert err <= 4e-6 * scale + 1e-12, f"update {i}: {key} differs by {err:.3e} (max |g| {scale:.3e})"
    for key in ("model_loss", "actor_loss", "value_loss"):
        np.testing.assert_allclose(b[key], a[key], rtol=2e-6, atol=1e-6, err_msg=key)
    assert torch.allclose(a["ema"], b["ema"], rtol=1e-6, atol=1e-7), (a["ema"], b["ema"])
    for k, v in a["params"].items():  # (learning rates 0: nothing moves but the slow critic, by the same EMA steps)
        assert torch.equal(v, b["params"][k]), k


@pytest.mark.parametrize("name", ["tiny_gauss", "cfg2_gauss"])
def test_graph_replay_equals_eager(name):
    """Learning rates 0 (the exact claim): every update's sampled states and actions bit-equal between eager launches
    and hipGraph replay, gradients equal up to the atomic summation order of the reverse scan."""
    n = 4
    _same_run(_run(name, n, "eager"), _run(name, n, "graph"), n)


def test_pipelined_updates_equal_serial_updates():
    """step_pipelined + flush at cfg2_gauss gives the serial result (learning rates 0 for the exact claim)."""
    n = 5
    a, b = _run("cfg2_gauss", n, "graph"), _run("cfg2_gauss", n, "pipe")
    assert b["pipe"], "the pipelined segments were never captured: serial would be compared with serial"
    assert not a["pipe"]
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

    def dataset():
        while True:
            yield GC.make_batch(name)

    agent = dreamer.Dreamer(Hh.obs_space(name), None, cfg, _Logger(), dataset()).to(cfg.device)
    w = GC.make_weights(name)
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


@pytest.mark.parametrize("tag", ["train", "eval"])
@pytest.mark.parametrize("name", ALL)
def test_policy_steps_match_the_reference(name, tag):
    """Three consecutive acting steps on two environments through Dreamer._policy (all reset at step 0, one env reset
    at step 1): sampled while training; with eval_state_mean, stoch = mean and the actor's mode."""
    g = G.gold(name)
    training = tag == "train"
    agent = _agent(name, eval_state_mean=not training)
    state = None
    for t, st in enumerate(GC.make_policy_inputs(name)):
        obs = {k: st[k] for k in ("image", "is_first", "is_terminal")}
        noise = _dev({k: st[k] for k in ("prior", "post", "act")})
        out, state = agent._policy(obs, state, training, noise=noise)
        latent, action = state
        pre = f"policy/{tag}/{t}/"
        assert set(latent) == set(STATE_KEYS)
        for k in STATE_KEYS:
            G.close(latent[k], g[pre + k], what=pre + k)
        if not training:
            assert torch.equal(latent["stoch"], latent["mean"])
        G.close(out["action"], g[pre + "action"], what=pre + "action")
        G.close(out["logprob"], g[pre + "logprob"], tol=2e-4, what=pre + "logprob")


@pytest.mark.parametrize("eval_state_mean", [False, True])
@pytest.mark.parametrize("name", ["tiny_gauss", "tiny_gauss_onehot"])
def test_policy_graph_replay_equals_eager(name, eval_state_mean):
    import tools

    agent = _agent(name, eval_state_mean)
    steps = GC.make_policy_inputs(name) + GC.make_policy_inputs(name, seed=1)[1:]
    outs = {}
    for mode in ("eager", "graph"):
        tools.default_rng(agent._config.device, seed=21)
        state, res = None, []
        for t, st in enumerate(steps):
            obs = {k: st[k] for k in ("image", "is_first", "is_terminal")}
            training = t != len(steps) - 1
            if mode == "eager":
                out, state = agent._policy_eager(obs, state, training)
            else:
                out, state = agent._policy(obs, state, training)
            res.append((out["action"].clone(), out["logprob"].clone(), {k: v.clone() for k, v in state[0].items()}))
        outs[mode] = res
    assert agent._policy_runner not in (None, False) and len(agent._policy_runner._sig) == 2
    for (a0, l0, s0), (a1, l1, s1) in zip(outs["eager"], outs["graph"]):
        assert set(s0) == set(s1) == set(STATE_KEYS)
        for k in STATE_KEYS:
            assert torch.allclose(s0[k], s1[k], atol=1e-6), k
        if eval_state_mean:
            assert torch.equal(s1["stoch"], s1["mean"])
        assert torch.allclose(a0, a1, atol=1e-6) and torch.allclose(l0, l1, atol=1e-5)


def test_plan2explore_keeps_constructing():
    import exploration

    cfg, wm, _ = G.build_models("tiny_gauss")
    cfg.disag_models, cfg.disag_layers, cfg.disag_units = 2, 2, 16
    p2e = exploration.Plan2Explore(cfg, wm, lambda f, s, a: wm.heads["reward"](f).mean())
    assert len(list(p2e.parameters())) > 0
