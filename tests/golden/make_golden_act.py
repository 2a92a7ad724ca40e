#!/usr/bin/env python3
"""Golden vectors of the layer-activation configurations (act / encoder.act / decoder.act other than SiLU), from the
REFERENCE itself (build container only; the .npz files written here are data and travel, the reference does not).

    python tests/golden/make_golden_act.py [--only NAME]
        # writes tests/golden/tiny_elu.npz, tiny_elu_video.npz, tiny_actmix.npz, tiny_gauss_tanh.npz, tiny_p2e_elu.npz

The reference import, its config loader, the noise tape and the hooks that replace its random draws are those of
make_golden.py (and the torch.softplus accommodation of make_golden_gauss.py); the shapes' `act` / `enc_act` / `dec_act`
keys become the reference's config keys `act` / `encoder.act` / `decoder.act`.

Stored per shape, as make_golden_gauss.py stores for a tiny shape: the world model's and the behaviour's outputs, losses
and metrics piece by piece, every gradient, two consecutive updates through the reference's own `_train` pair (train/*,
after/*, train2/*, after2/*), and policy/*: three consecutive acting steps on two environments (sampled; for continuous
latents also with stoch = mean and the actor's mode).  tiny_p2e_elu holds, in the same file, two consecutive
exploration updates of the reference's exploration.Plan2Explore (p2e/*), as make_golden.py's run_p2e stores one.
tiny_elu_video.npz is WorldModel.video_pred's output.

ReLU (tiny_actmix's decoder): the generator records every ReLU module's input over the whole run and asserts that none
lies within act_common.RELU_MARGIN (1e-4) of zero, so that a rounding difference cannot flip a gradient; otherwise it
moves to the next weight seed.  Seed used for the committed fixture: 43 (act_common.WEIGHT_SEED; seeds 0..42 each put
a pre-activation within the margin), smallest |input| of that run 1.463e-04 (the fixture's meta/relu_min).
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import act_common as AC  # noqa: E402
from tests.golden import common  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden.make_golden import ObsSpace, Space, Tape, import_reference, install_noise_hooks, load_config  # noqa: E402


def to_np(x):
    """A COPY: the reference writes into tensors it was handed after their values have been put aside here."""
    return x.detach().cpu().numpy().copy()


class ReluWatch:
    """Smallest |input| any nn.ReLU module of the given models saw."""

    def __init__(self, *mods):
        self.min = np.inf
        for m in mods:
            for sub in m.modules():
                if isinstance(sub, torch.nn.ReLU):
                    sub.register_forward_hook(self._hook)

    def _hook(self, mod, inp, out):
        self.min = min(self.min, float(inp[0].detach().abs().min()))


def build_reference(name, models):
    s = common.SHAPES[name]
    ov = dict(
        device="cpu", compile=False, num_actions=s["A"], dyn_stoch=s["stoch"], dyn_discrete=s["discrete"],
        dyn_deter=s["deter"], dyn_hidden=s["hidden"], units=s["units"], batch_size=s["B"], batch_length=s["T"],
        imag_horizon=s["H"], imag_gradient=s["imag_gradient"], act=s["act"],
        encoder=dict(cnn_depth=s["cnn_depth"], act=s["enc_act"]), decoder=dict(cnn_depth=s["cnn_depth"], act=s["dec_act"]),
        causal_world_model=False, imag_gradient_mix=0.0, actor=dict(layers=2), critic=dict(layers=2),
        reward_head=dict(layers=2), cont_head=dict(layers=2),
    )
    for key in ("mean_act", "std_act", "min_std"):
        if key in s:
            ov["dyn_" + key] = s[key]
    if "p2e" in s:
        ov.update(expl_behavior="plan2explore", **s["p2e"])
    if s["actor_dist"] == "onehot":
        ov["actor"].update(dist="onehot", std="none")
    spaces = {}
    if s["encoder"] in ("mlp", "both"):
        keys = "|".join(k for k, _ in common.PROPRIO_KEYS)
        for d in (ov["encoder"], ov["decoder"]):
            d.update(mlp_units=s["enc_mlp_units"], mlp_layers=s["enc_mlp_layers"], mlp_keys=keys, cnn_keys="image")
        for k, w in common.PROPRIO_KEYS:
            spaces[k] = Space((w,))
    cfg = load_config(["dmc_vision"], ov)
    spaces.update(image=Space((64, 64, 3)), is_first=Space((1,)), is_terminal=Space((1,)))
    with contextlib.redirect_stdout(io.StringIO()):
        wm = models.WorldModel(ObsSpace(spaces), None, 0, cfg)
        beh = models.ImagBehavior(cfg, wm)
    # the activation modules are what the shape asks for, key by key
    names = lambda m: {type(x).__name__ for x in m.modules()} & set(("SiLU", "ReLU", "ELU", "GELU", "Tanh", "Mish"))
    assert names(wm.encoder) == {s["enc_act"]}, names(wm.encoder)
    assert names(wm.heads["decoder"]) == {s["dec_act"]}, names(wm.heads["decoder"])
    assert names(wm.dynamics) == names(wm.heads["reward"]) == names(beh.actor) == {s["act"]}
    wm.requires_grad_(False)
    beh.requires_grad_(False)
    w = AC.make_weights(name)
    sd_wm = {k: torch.from_numpy(v) for k, v in w.items() if k.split(".")[0] in ("encoder", "dynamics", "heads")}
    ref_sd = wm.state_dict()
    assert set(ref_sd) == set(sd_wm), set(ref_sd) ^ set(sd_wm)
    for k, v in sd_wm.items():
        assert tuple(ref_sd[k].shape) == tuple(v.shape), (k, ref_sd[k].shape, v.shape)
    wm.load_state_dict(sd_wm)
    sd_beh = beh.state_dict()
    own = {k for k in sd_beh if not k.startswith("_world_model.") and k != "ema_vals"}
    assert own == {k for k in w if k.split(".")[0] in ("actor", "value", "_slow_value")}
    for k in own:
        sd_beh[k] = torch.from_numpy(w[k])
    beh.load_state_dict(sd_beh)
    return cfg, wm, beh, w


def run_policy(name, wm, actor, steps, training):
    """dreamer.py:116-166 -> per-step dict(action, logprob, <state keys>).  training=False: eval_state_mean (continuous
    latents only)."""
    quiet = contextlib.redirect_stdout(io.StringIO())
    latent = action = None
    outs = []
    for st in steps:
        MG.TAPE = Tape([st["prior"], st["post"]] + ([st["act"]] if training else []))
        with torch.no_grad(), quiet:
            obs = wm.preprocess({k: st[k].copy() for k in AC.obs_keys(name)})
            embed = wm.encoder(obs)
            latent, _ = wm.dynamics.obs_step(latent, action, embed, obs["is_first"])
            if not training:
                latent["stoch"] = latent["mean"]
            feat = wm.dynamics.get_feat(latent)
            dist = actor(feat)
            action = dist.sample() if training else dist.mode()
            logprob = dist.log_prob(action)
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        latent = {k: v.detach() for k, v in latent.items()}
        action = action.detach()
        outs.append(dict(action=to_np(action), logprob=to_np(logprob), **{k: to_np(v) for k, v in latent.items()}))
    MG.TAPE = None
    return outs


WM_METS = ("model_loss", "model_grad_norm", "kl", "prior_ent", "post_ent", "dyn_loss", "rep_loss", "reward_loss",
           "cont_loss")
BEH_METS = ("actor_loss", "actor_grad_norm", "value_loss", "value_grad_norm", "actor_entropy", "EMA_005", "EMA_095",
            "target_mean", "target_std", "imag_reward_mean", "value_mean")


def run_config(name, models):
    """-> (dict of arrays, smallest |ReLU input| of the run)."""
    s = common.SHAPES[name]
    S = AC.src(name)
    skeys = AC.state_keys(name)
    cfg, wm, beh, w = build_reference(name, models)
    watch = ReluWatch(wm, beh)
    data = AC.make_batch(name)
    noise = AC.make_noise(name)
    out = {}
    quiet = contextlib.redirect_stdout(io.StringIO())

    def keep(key, arr):
        arr = np.asarray(arr)
        out["sum/" + key] = common.checksum(arr)
        out[key] = arr

    # ---- acting steps (weights as loaded) ---------------------------------------------------------
    steps = AC.make_policy_inputs(name)
    for tag, training in (("train", True),) + ((("eval", False),) if AC.gauss(name) else ()):
        for t, o in enumerate(run_policy(name, wm, beh.actor, steps, training)):
            for k, v in o.items():
                out[f"policy/{tag}/{t}/{k}"] = v

    # ---- world model forward, piece by piece ---------------------------------------------------------
    for prm in list(wm.parameters()) + list(beh.parameters()):
        prm.requires_grad_(True)
    MG.TAPE = Tape(S.observe_tape(noise))
    with quiet:
        obs = wm.preprocess({k: v.copy() for k, v in data.items()})
    embed = wm.encoder(obs)
    action_in = obs["action"].clone()
    post, prior = wm.dynamics.observe(embed, action_in, obs["is_first"])
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    assert set(post) == set(skeys), set(post)
    kl_loss, kl_value, dyn_loss, rep_loss = wm.dynamics.kl_loss(post, prior, cfg.kl_free, cfg.dyn_scale, cfg.rep_scale)
    klv = to_np(kl_value)
    n_clip, n_free = int((klv < cfg.kl_free).sum()), int((klv > cfg.kl_free).sum())
    print(f"[golden] {name}: per-step KL min {klv.min():.3f} max {klv.max():.3f}; {n_clip} clipped at kl_free, "
          f"{n_free} above")
    if AC.gauss(name):
        assert n_clip >= 1 and n_free >= 1, "scale gauss_common.STAT_SCALE until the KL values straddle kl_free"
    feat = wm.dynamics.get_feat(post)
    losses, preds = {}, {}
    for hname, head in wm.heads.items():
        pred = head(feat)
        if isinstance(pred, dict):
            preds.update(pred)
        else:
            preds[hname] = pred
    for k, pred in preds.items():
        losses[k] = -pred.log_prob(obs[k])
    model_loss = torch.mean(sum(losses.values()) + kl_loss)
    wm_params = dict(wm.named_parameters())
    grads = torch.autograd.grad(model_loss, list(wm_params.values()), allow_unused=True)

    keep("embed", to_np(embed))
    for k in skeys:
        keep("post/" + k, to_np(post[k]))
        keep("prior/" + k, to_np(prior[k]))
    keep("action_after", to_np(action_in))
    recon = to_np(preds["image"].mode())
    out["sum/recon"] = common.checksum(recon)
    out["recon"] = recon[0:1, 0:2]
    if s["encoder"] in ("mlp", "both"):
        for k, _ in common.PROPRIO_KEYS:
            keep("recon/" + k, to_np(preds[k]._mode))
    keep("reward_logits", to_np(preds["reward"].logits))
    keep("cont_logit", to_np(preds["cont"]._dist.base_dist.logits))
    for k, v in losses.items():
        out["loss/" + k] = to_np(v)
    out["kl_value"], out["dyn_loss"], out["rep_loss"] = klv, to_np(dyn_loss), to_np(rep_loss)
    out["kl_loss"] = to_np(kl_loss)
    out["model_loss"] = to_np(model_loss)
    out["prior_ent"] = to_np(wm.dynamics.get_dist(prior).entropy())
    out["post_ent"] = to_np(wm.dynamics.get_dist(post).entropy())
    gn = 0.0
    for (k, _), g in zip(wm_params.items(), grads):
        assert g is not None, k
        keep("grad/" + k, to_np(g))
        gn += float((g.double() ** 2).sum())
    out["model_grad_norm"] = np.float64(np.sqrt(gn))

    # ---- behaviour forward -------------------------------------------------------------------------
    start = {k: v.detach() for k, v in post.items()}
    objective = lambda f, st, a: wm.heads["reward"](wm.dynamics.get_feat(st)).mode()  # dreamer.py:196-198
    MG.TAPE = Tape(S.imagine_tape(noise))
    feats, states, actions = beh._imagine(start, beh.actor, cfg.imag_horizon)
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    keep("imag/feat", to_np(feats))
    keep("imag/action", to_np(actions))
    for k in skeys:
        keep("imag/" + k, to_np(states[k]))
    reward = objective(feats, states, actions)
    actor_ent = beh.actor(feats).entropy()
    ema0 = beh.ema_vals.clone()
    target, weights, base = beh._compute_target(feats, states, reward)
    actor_loss, mets = beh._compute_actor_loss(feats, actions, target, weights, base)
    actor_loss = torch.mean(actor_loss - cfg.actor["entropy"] * actor_ent[:-1, ..., None])
    value = beh.value(feats[:-1].detach())
    tgt = torch.stack(target, dim=1)
    value_loss = -value.log_prob(tgt.detach())
    slow = beh._slow_value(feats[:-1].detach())
    value_loss = value_loss - value.log_prob(slow.mode().detach())
    value_loss = torch.mean(weights[:-1] * value_loss[:, :, None])
    keep("imag/reward", to_np(reward))
    keep("imag/actor_ent", to_np(actor_ent))
    keep("imag/target", to_np(tgt))
    keep("imag/weights", to_np(weights))
    keep("imag/value", to_np(beh.value(feats).mode()))
    out["ema_vals_after"], out["ema_vals_before"] = to_np(beh.ema_vals), to_np(ema0)
    out["actor_loss"], out["value_loss"] = to_np(actor_loss), to_np(value_loss)
    a_params, v_params = dict(beh.actor.named_parameters()), dict(beh.value.named_parameters())
    ga = torch.autograd.grad(actor_loss, list(a_params.values()), retain_graph=True)
    gv = torch.autograd.grad(value_loss, list(v_params.values()))
    for (k, _), g in zip(a_params.items(), ga):
        keep("grad/actor." + k, to_np(g))
    for (k, _), g in zip(v_params.items(), gv):
        keep("grad/value." + k, to_np(g))
    out["actor_grad_norm"] = np.float64(np.sqrt(sum(float((g.double() ** 2).sum()) for g in ga)))
    out["value_grad_norm"] = np.float64(np.sqrt(sum(float((g.double() ** 2).sum()) for g in gv)))

    # ---- two consecutive updates through the reference's own _train pair ----------------------------------
    for prm in list(wm.parameters()) + list(beh.parameters()):
        prm.requires_grad_(False)
    beh.ema_vals.copy_(ema0)
    reward_fn = lambda f, st, a: wm.heads["reward"](wm.dynamics.get_feat(st)).mode()
    for i, (tr, af) in enumerate((("train/", "after/"), ("train2/", "after2/"))):
        d_i = data if i == 0 else AC.make_batch(name, seed=i)
        n_i = noise if i == 0 else AC.make_noise(name, seed=i)
        MG.TAPE = Tape(S.observe_tape(n_i))
        with quiet:
            post_t, context, mets_wm = wm._train({k: v.copy() for k, v in d_i.items()})
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        for k in WM_METS + tuple(k + "_loss" for k in losses if k not in ("reward", "cont")):
            out[tr + k] = np.asarray(mets_wm[k], np.float64)
        if i == 0:
            assert torch.equal(post_t["stoch"], post["stoch"].detach())
        keep(tr + "post/stoch", to_np(post_t["stoch"]))
        keep(tr + "post/deter", to_np(post_t["deter"]))
        MG.TAPE = Tape(S.imagine_tape(n_i))
        with quiet:
            bres = beh._train(post_t, reward_fn)
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        mets_b = bres[-1]
        keep(tr + "imag/stoch", to_np(bres[1]["stoch"]))
        keep(tr + "imag/action", to_np(bres[2]))
        for k in BEH_METS:
            out[tr + k] = np.asarray(mets_b[k], np.float64)
        sd = {**dict(wm.state_dict()), **{k: v for k, v in beh.state_dict().items() if not k.startswith("_world_model.")}}
        for k, v in sd.items():
            keep(af + k, to_np(v))
    MG.TAPE = None
    out["meta/name"] = np.array(name)
    out["meta/full"] = np.array(True)
    out["meta/weight_seed"] = np.array(AC.WEIGHT_SEED.get(name, 0))
    out["meta/relu_min"] = np.float64(watch.min)
    return out, watch.min


def run_p2e(name, models, out):
    """Two consecutive rounds of dreamer.py:194-203 with expl_behavior plan2explore: wm._train(data) -> p2e.train(start,
    context, data), as make_golden.py's run_p2e does once.  Adds p2e/* to `out`."""
    sys.path.insert(0, MG.REF)
    import exploration

    cfg, wm, beh, w = build_reference(name, models)
    extr = lambda f, st, a: wm.heads["reward"](f).mean()  # dreamer.py:80
    with contextlib.redirect_stdout(io.StringIO()):
        p2e = exploration.Plan2Explore(cfg, wm, extr)
    assert {type(x).__name__ for x in p2e._networks.modules()} >= {common.SHAPES[name]["act"]}
    p2e.requires_grad_(False)
    pw = common.make_p2e_weights(name)
    sd = p2e.state_dict()
    own = {k for k in sd if not k.startswith(("_behavior._world_model.", "actor.")) and k != "_behavior.ema_vals"}
    assert own == set(pw), own ^ set(pw)
    for k in own:
        assert tuple(sd[k].shape) == pw[k].shape, (k, sd[k].shape, pw[k].shape)
        sd[k] = torch.from_numpy(pw[k])
        if k.startswith("_behavior.actor."):
            sd[k[len("_behavior."):]] = sd[k]
    p2e.load_state_dict(sd)
    quiet = contextlib.redirect_stdout(io.StringIO())
    grabbed = {}

    def grab(tag, named):
        def hook(opt, args, kwargs):
            for k, prm in named:
                grabbed[f"{tag}{k}"] = prm.grad.detach().clone()
        return hook

    p2e._expl_opt._opt.register_step_pre_hook(grab("_networks.", list(p2e._networks.named_parameters())))
    p2e._behavior._actor_opt._opt.register_step_pre_hook(grab("_behavior.actor.", list(p2e._behavior.actor.named_parameters())))
    p2e._behavior._value_opt._opt.register_step_pre_hook(grab("_behavior.value.", list(p2e._behavior.value.named_parameters())))
    seen = {}
    stock_reward = p2e._intrinsic_reward

    def spy(feat, state, action):
        r = stock_reward(feat, state, action)
        seen["reward"], seen["feat"], seen["action"] = r.detach().clone(), feat.detach().clone(), action.detach().clone()
        return r

    p2e._intrinsic_reward = spy
    for i, (tr, gr, af) in enumerate((("p2e/train/", "p2e/grad/", "p2e/after/"), ("p2e/train2/", "p2e/grad2/", "p2e/after2/"))):
        data = AC.make_batch(name, seed=i)
        noise = AC.make_noise(name, seed=i)
        noise_x = AC.make_noise(name, seed=5 + i)  # the exploration behaviour's own imagination draws
        MG.TAPE = Tape(common.observe_tape(noise))
        with quiet:
            post, context, _ = wm._train({k: v.copy() for k, v in data.items()})
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        MG.TAPE = Tape(common.imagine_tape(noise_x))
        with quiet:
            _, mets = p2e.train(post, context, {k: v.copy() for k, v in data.items()})
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        MG.TAPE = None
        for k in ("explorer_loss", "explorer_grad_norm", "actor_loss", "actor_grad_norm", "value_loss", "value_grad_norm",
                  "actor_entropy", "EMA_005", "EMA_095", "imag_reward_mean", "imag_reward_std", "target_mean",
                  "value_mean"):
            out[tr + k] = np.asarray(mets[k], np.float64)
        out[tr + "imag/reward"] = to_np(seen["reward"])
        out[tr + "imag/feat"] = to_np(seen["feat"])
        out[tr + "imag/action"] = to_np(seen["action"])
        out[tr + "post/stoch"], out[tr + "post/deter"] = to_np(post["stoch"]), to_np(post["deter"])
        for k, g in grabbed.items():
            out[gr + k] = to_np(g)
        for k, v in p2e.state_dict().items():
            if not k.startswith(("_behavior._world_model.", "actor.")):
                out[af + k] = to_np(v)
        # (the world model's own parameters after this round are after/* resp. after2/* of run_config: same batch, noise)


def run_video(name, models):
    cfg, wm, beh, w = build_reference(name, models)
    data = AC.make_batch(name)
    noise = AC.src(name).make_video_noise(name)
    MG.TAPE = Tape(AC.src(name).video_tape(noise))
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        video = wm.video_pred({k: v.copy() for k, v in data.items()})
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    MG.TAPE = None
    v = to_np(video)
    # rows: truth | model | error, 64 pixels each (models.py:213); the truth third is the input image and not stored
    out = {"sum/video": common.checksum(v), "meta/shape": np.array(v.shape), "video_model": v[:, :, 64:128].astype(np.float32)}
    path = os.path.join(HERE, f"{name}_video.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, video {v.shape}, mean {v.mean():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    tools, networks, models = import_reference()
    install_noise_hooks(tools)
    if not hasattr(torch, "softplus"):
        torch.softplus = torch.nn.functional.softplus
    for name in AC.NAMES:
        if args.only not in (None, name):
            continue
        relu = "ReLU" in (common.SHAPES[name][k] for k in ("act", "enc_act", "dec_act"))
        while True:
            out, rmin = run_config(name, models)
            if not relu:
                break
            print(f"[golden] {name}: weight seed {AC.WEIGHT_SEED.get(name, 0)}, smallest |ReLU input| {rmin:.3e}")
            if rmin > AC.RELU_MARGIN:
                break
            AC.WEIGHT_SEED[name] = AC.WEIGHT_SEED.get(name, 0) + 1
        if name == AC.P2E:
            run_p2e(name, models, out)
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"[golden] wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays; "
              f"model_loss={float(out['model_loss']):.6f} actor_loss={float(out['actor_loss']):.6f} "
              f"value_loss={float(out['value_loss']):.6f}")
    if args.only in (None, "tiny_elu_video"):
        run_video("tiny_elu", models)


if __name__ == "__main__":
    main()
