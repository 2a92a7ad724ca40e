#!/usr/bin/env python3
"""Golden vectors of the continuous-latent configurations (dyn_discrete: 0), from the REFERENCE itself
(build container only; the .npz files written here are data and travel, the reference does not).

    python tests/golden/make_golden_gauss.py [--only NAME]     # writes tests/golden/<name>.npz, tiny_gauss_video.npz

The reference import, its config loader, the noise tape and the hooks that replace its random draws are those of
make_golden.py; every Gaussian draw of the reference goes through torch.distributions.normal._standard_normal, which
install_noise_hooks replaces by the tape.  One more import accommodation: the reference's `softplus` std activation
calls `torch.softplus`, which torch does not have (networks.py:264); torch.nn.functional.softplus is bound to that name
while the generator runs.

Stored, in addition to what make_golden.py stores for the discrete shapes (with mean / std in place of logit): a second
consecutive update with batch and noise seed 1 (train2/*, after2/*), and policy/*: three consecutive acting steps on two
environments through encoder -> dynamics.obs_step -> actor (dreamer.py:116-166), sampled (training) and with
stoch = mean and actor.mode() (eval_state_mean).  Images and weights of the tiny shapes are regenerated from
gauss_common by the tests (the weights are stored too, as w/*); the stored reconstruction is a slice plus a checksum.
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

from tests.golden import common, gauss_common as GC  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden.make_golden import ObsSpace, Space, Tape, import_reference, install_noise_hooks, load_config  # noqa: E402


def build_reference(name, models):
    s = common.SHAPES[name]
    ov = dict(
        device="cpu", compile=False, num_actions=s["A"], dyn_stoch=s["stoch"], dyn_discrete=0, dyn_deter=s["deter"],
        dyn_hidden=s["hidden"], units=s["units"], batch_size=s["B"], batch_length=s["T"], imag_horizon=s["H"],
        imag_gradient=s["imag_gradient"], encoder=dict(cnn_depth=s["cnn_depth"]), decoder=dict(cnn_depth=s["cnn_depth"]),
        causal_world_model=False, imag_gradient_mix=0.0, actor=dict(layers=2), critic=dict(layers=2),
        reward_head=dict(layers=2), cont_head=dict(layers=2),
    )
    for key in ("mean_act", "std_act", "min_std"):
        if key in s:
            ov["dyn_" + key] = s[key]
    if s["actor_dist"] == "onehot":
        ov["actor"].update(dist="onehot", std="none")
    cfg = load_config(["dmc_vision"], ov)
    spaces = {"image": Space((64, 64, 3)), "is_first": Space((1,)), "is_terminal": Space((1,))}
    with contextlib.redirect_stdout(io.StringIO()):
        wm = models.WorldModel(ObsSpace(spaces), None, 0, cfg)
        beh = models.ImagBehavior(cfg, wm)
    wm.requires_grad_(False)
    beh.requires_grad_(False)
    w = GC.make_weights(name)
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


def to_np(x):
    """A COPY: the reference writes into tensors it was handed (obs_step zeroes prev_action in place, the optimizers
    update the parameters in place) after their values have been put aside here."""
    return x.detach().cpu().numpy().copy()


def run_policy(wm, beh, steps, training):
    """dreamer.py:116-166 with the task actor: -> per-step dict(action, logprob, stoch, deter, mean, std)."""
    quiet = contextlib.redirect_stdout(io.StringIO())
    latent = action = None
    outs = []
    for st in steps:
        MG.TAPE = Tape([st["prior"], st["post"]] + ([st["act"]] if training else []))
        with torch.no_grad(), quiet:
            obs = wm.preprocess({k: st[k].copy() for k in ("image", "is_first", "is_terminal")})
            embed = wm.encoder(obs)
            latent, _ = wm.dynamics.obs_step(latent, action, embed, obs["is_first"])
            if not training:  # eval_state_mean (dreamer.py:129-131)
                latent["stoch"] = latent["mean"]
            feat = wm.dynamics.get_feat(latent)
            actor = beh.actor(feat)
            action = actor.sample() if training else actor.mode()
            logprob = actor.log_prob(action)
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        latent = {k: v.detach() for k, v in latent.items()}
        action = action.detach()
        outs.append(dict(action=to_np(action), logprob=to_np(logprob), **{k: to_np(v) for k, v in latent.items()}))
    MG.TAPE = None
    return outs


def run_config(name, models, full: bool):
    s = common.SHAPES[name]
    cfg, wm, beh, w = build_reference(name, models)
    data = GC.make_batch(name)
    noise = GC.make_noise(name)
    out = {}
    samples, deltas = {}, {}  # group ("grad", "after", "after2") -> {parameter name: sampled elements / delta checksum}
    quiet = contextlib.redirect_stdout(io.StringIO())

    def keep(key, arr, rows=None, force_rows=False):
        arr = np.asarray(arr)
        out["sum/" + key] = common.checksum(arr)
        if full and not force_rows:
            out[key] = arr
        elif rows is not None:
            out[key] = arr[rows]

    def keep_param(key, arr, name):
        """A gradient or an Adam-updated parameter: everything for the tiny shapes; for the full-size one the checksum
        plus the elements gauss_common.sample_index(name) picks (the same elements of grad, after and after2)."""
        arr = np.asarray(arr)
        keep(key, arr)
        if not full:
            samples.setdefault(key.split("/")[0], {})[name] = arr.reshape(-1)[GC.sample_index(name, arr.size)]

    # ---- acting steps (weights as loaded) ---------------------------------------------------------
    steps = GC.make_policy_inputs(name)
    for tag, training in (("train", True), ("eval", False)):
        for t, o in enumerate(run_policy(wm, beh, steps, training)):
            for k, v in o.items():
                out[f"policy/{tag}/{t}/{k}"] = v

    # ---- world model forward, piece by piece ---------------------------------------------------------
    for prm in list(wm.parameters()) + list(beh.parameters()):
        prm.requires_grad_(True)
    MG.TAPE = Tape(GC.observe_tape(noise))
    with quiet:
        obs = wm.preprocess({k: v.copy() for k, v in data.items()})
    embed = wm.encoder(obs)
    action_in = obs["action"].clone()
    post, prior = wm.dynamics.observe(embed, action_in, obs["is_first"])
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    assert set(post) == {"stoch", "deter", "mean", "std"}, set(post)
    kl_loss, kl_value, dyn_loss, rep_loss = wm.dynamics.kl_loss(post, prior, cfg.kl_free, cfg.dyn_scale, cfg.rep_scale)
    # free-bits coverage: both sides of the clip are exercised
    klv = to_np(kl_value)
    n_clip, n_free = int((klv < cfg.kl_free).sum()), int((klv > cfg.kl_free).sum())
    print(f"[golden] {name}: per-step KL min {klv.min():.3f} max {klv.max():.3f}; {n_clip} clipped at kl_free, "
          f"{n_free} above")
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

    sel = slice(0, 2) if full else slice(0, 1)  # (slices of the full-size shape: every fixture stays below 1 MiB)
    keep("embed", to_np(embed), (sel, slice(0, 8)))
    for k in ("stoch", "deter", "mean", "std"):
        keep("post/" + k, to_np(post[k]), sel)
        if full or k != "deter":  # (prior deter IS post deter, networks.py:205: not stored twice at full size)
            keep("prior/" + k, to_np(prior[k]), sel)
    keep("action_after", to_np(action_in))
    keep("recon", to_np(preds["image"].mode()), (slice(0, 1), slice(0, 2)), force_rows=True)
    keep("reward_logits", to_np(preds["reward"].logits), sel)
    keep("cont_logit", to_np(preds["cont"]._dist.base_dist.logits), sel)
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
        keep_param("grad/" + k, to_np(g), k)
        gn += float((g.double() ** 2).sum())
    out["model_grad_norm"] = np.float64(np.sqrt(gn))

    # ---- behaviour forward -------------------------------------------------------------------------
    start = {k: v.detach() for k, v in post.items()}
    objective = lambda f, st, a: wm.heads["reward"](wm.dynamics.get_feat(st)).mode()  # dreamer.py:196-198
    MG.TAPE = Tape(GC.imagine_tape(noise))
    feats, states, actions = beh._imagine(start, beh.actor, cfg.imag_horizon)
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    rows = (slice(None), slice(0, 8 if full else 4))
    keep("imag/feat", to_np(feats), rows)
    keep("imag/action", to_np(actions), rows)
    for k in ("stoch", "deter", "mean", "std"):
        keep("imag/" + k, to_np(states[k]), rows)
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
    keep("imag/reward", to_np(reward), rows)
    keep("imag/actor_ent", to_np(actor_ent), rows)
    keep("imag/target", to_np(tgt), rows)
    keep("imag/weights", to_np(weights), rows)
    keep("imag/value", to_np(beh.value(feats).mode()), rows)
    out["ema_vals_after"], out["ema_vals_before"] = to_np(beh.ema_vals), to_np(ema0)
    out["actor_loss"], out["value_loss"] = to_np(actor_loss), to_np(value_loss)
    a_params, v_params = dict(beh.actor.named_parameters()), dict(beh.value.named_parameters())
    ga = torch.autograd.grad(actor_loss, list(a_params.values()), retain_graph=True)
    gv = torch.autograd.grad(value_loss, list(v_params.values()))
    for (k, _), g in zip(a_params.items(), ga):
        keep_param("grad/actor." + k, to_np(g), "actor." + k)
    for (k, _), g in zip(v_params.items(), gv):
        keep_param("grad/value." + k, to_np(g), "value." + k)
    out["actor_grad_norm"] = np.float64(np.sqrt(sum(float((g.double() ** 2).sum()) for g in ga)))
    out["value_grad_norm"] = np.float64(np.sqrt(sum(float((g.double() ** 2).sum()) for g in gv)))

    # ---- two consecutive updates through the reference's own _train pair ----------------------------------
    for prm in list(wm.parameters()) + list(beh.parameters()):
        prm.requires_grad_(False)
    beh.ema_vals.copy_(ema0)
    reward_fn = lambda f, st, a: wm.heads["reward"](wm.dynamics.get_feat(st)).mode()
    for i, (tr, af) in enumerate((("train/", "after/"), ("train2/", "after2/"))):
        d_i = data if i == 0 else GC.make_batch(name, seed=i)
        n_i = noise if i == 0 else GC.make_noise(name, seed=i)
        MG.TAPE = Tape(GC.observe_tape(n_i))
        with quiet:
            post_t, context, mets_wm = wm._train({k: v.copy() for k, v in d_i.items()})
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        for k in ("model_loss", "model_grad_norm", "kl", "prior_ent", "post_ent", "dyn_loss", "rep_loss", "image_loss",
                  "reward_loss", "cont_loss"):
            out[tr + k] = np.asarray(mets_wm[k], np.float64)
        if i == 0:
            assert torch.equal(post_t["mean"], post["mean"].detach())
        MG.TAPE = Tape(GC.imagine_tape(n_i))
        with quiet:
            mets_b = beh._train(post_t, reward_fn)[-1]
        assert MG.TAPE.pos == len(MG.TAPE.arrays)
        for k in ("actor_loss", "actor_grad_norm", "value_loss", "value_grad_norm", "actor_entropy", "EMA_005", "EMA_095",
                  "target_mean", "target_std", "imag_reward_mean", "value_mean"):
            out[tr + k] = np.asarray(mets_b[k], np.float64)
        sd = {**dict(wm.state_dict()), **{k: v for k, v in beh.state_dict().items() if not k.startswith("_world_model.")}}
        for k, v in sd.items():
            keep_param(af + k, to_np(v), k)
            if not full and k in w:  # what the update did to the parameter: after - before (before: after/ for after2/)
                before = w[k] if i == 0 else prev_sd[k]
                deltas.setdefault(af[:-1], {})[k] = common.checksum(to_np(v).astype(np.float64) - before.astype(np.float64))
        prev_sd = {k: to_np(v) for k, v in sd.items()}
    MG.TAPE = None

    out["meta/name"] = np.array(name)
    out["meta/full"] = np.array(full)
    if full:
        for k, v in data.items():
            if k != "image":  # (regenerated by gauss_common.make_batch: 221 KB of incompressible bytes)
                out["data/" + k] = v
        out["sum/data/image"] = common.checksum(data["image"])
        for k, v in noise.items():
            out["noise/" + k] = v
        for k, v in w.items():
            out["w/" + k] = v
    else:
        # one array per group, the parameters in sorted order (gauss_common.sample_layout gives the offsets)
        for grp, d in samples.items():
            out["smp/" + grp] = np.concatenate([d[k] for k in sorted(d)]).astype(np.float32)
        for grp, d in deltas.items():
            out["sum/delta/" + grp] = np.stack([d[k] for k in sorted(d)])
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays; "
          f"model_loss={float(out['model_loss']):.6f} actor_loss={float(out['actor_loss']):.6f} "
          f"value_loss={float(out['value_loss']):.6f}")


def run_video(name, models):
    cfg, wm, beh, w = build_reference(name, models)
    data = GC.make_batch(name)
    noise = GC.make_video_noise(name)
    MG.TAPE = Tape(GC.video_tape(noise))
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
    for name, full in (("tiny_gauss", True), ("tiny_gauss_onehot", True), ("cfg2_gauss", False)):
        if args.only in (None, name):
            run_config(name, models, full)
    if args.only in (None, "tiny_gauss_video"):
        run_video("tiny_gauss", models)


if __name__ == "__main__":
    main()
