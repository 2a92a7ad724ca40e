"""Scaffolding of the layer-activation tests (act / encoder.act / decoder.act other than SiLU; fixtures written by
tests/golden/make_golden_act.py from the reference): models with the fixture's weights, its noise on the device in the
GPU path's row order, teacher-forcing inputs for the categorical draws, and the list of fixture keys the path test reads.

The comparisons themselves are tests/gauss_helpers.py's (close 1e-4, grad_close at grad_tol: 5e-6 of the tensor's max
for the actor's and the critic's tensors, GRAD_BOUND for the world model's against the reference's CPU vectors,
adam_close 1e-6), imported by the tests and not restated here."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import helpers as Hh
from tests.golden import act_common as AC
from tests.golden import common

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WM_METRICS = ("kl", "prior_ent", "post_ent", "dyn_loss", "rep_loss", "reward_loss", "cont_loss")
BEH_METRICS = ("actor_loss", "value_loss", "actor_entropy", "EMA_005", "EMA_095", "target_mean", "target_std",
               "imag_reward_mean", "value_mean")
NORMS = ("model_grad_norm", "actor_grad_norm", "value_grad_norm")
P2E_METRICS = ("explorer_loss", "explorer_grad_norm", "actor_loss", "actor_grad_norm", "value_loss", "value_grad_norm",
               "actor_entropy", "EMA_005", "EMA_095", "imag_reward_mean", "target_mean")


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def build_models(name, device="cuda:0"):
    return Hh.build_models(name, device, weights=AC.make_weights(name))


def decoder_keys(name):
    """Keys whose -log_prob the decoder contributes (the image, and the vector keys of a shape that has them)."""
    s = common.SHAPES[name]
    return ["image"] + ([k for k, _ in common.PROPRIO_KEYS] if s["encoder"] in ("mlp", "both") else [])


def param_names(name):
    return list(AC.src(name).param_shapes(name))


def fixture_keys(name):
    """Every key tests/test_act_path_gpu.py reads from tests/golden/<name>.npz."""
    sk = AC.state_keys(name)
    keys = ["meta/full", "model_loss", "model_grad_norm", "actor_loss", "value_loss", "ema_vals_after", "kl_value"]
    keys += [f"{p}/{k}" for p in ("post", "prior", "imag") for k in sk]
    keys += ["imag/action", "imag/feat", "imag/weights", "imag/reward", "imag/target", "imag/value", "imag/actor_ent"]
    for k in param_names(name):
        if not k.startswith("_slow_value."):
            keys.append("grad/" + k)
        keys += ["after/" + k, "after2/" + k]
    for tr in ("train/", "train2/"):
        keys += [tr + k for k in ("model_loss",) + WM_METRICS + BEH_METRICS + NORMS]
        keys += [tr + k + "_loss" for k in decoder_keys(name)]
        keys += [tr + "post/stoch", tr + "post/deter", tr + "imag/stoch", tr + "imag/action"]
    tags = ("train", "eval") if AC.gauss(name) else ("train",)
    keys += [f"policy/{tag}/{t}/{k}" for tag in tags for t in range(AC.POLICY_STEPS) for k in sk + ("action", "logprob")]
    if name == AC.P2E:
        for i, (tr, gr, af) in enumerate((("p2e/train/", "p2e/grad/", "p2e/after/"), ("p2e/train2/", "p2e/grad2/", "p2e/after2/"))):
            keys += [tr + k for k in P2E_METRICS + ("imag/reward", "imag/feat", "imag/action")]
            for k in common.p2e_param_shapes(name):
                if not k.startswith("_behavior._slow_value."):
                    keys.append(gr + k)
                keys.append(af + k)
    return keys


def onehot_index(x):
    return torch.from_numpy(np.asarray(x)).argmax(-1).to(torch.int32).contiguous()


def gpu_noise(name, seed=0, g=None, tr=None, flips=None, imag_stoch=None, imag_action=None, prior=True):
    """(wm_noise, im_noise) for WorldModel._train / ImagBehavior._train.  With a fixture g (categorical latents): the
    draws are teacher-forced to the reference's classes -- the posterior's g[tr + "post/stoch"] (and, prior=True, the
    prior's g["prior/stoch"]), the imagination's imag_stoch [H,N,S,D] / imag_action [H,N,A] (default g[tr + "imag/..."])
    -- and `flips` counts the draws that would have differed."""
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    n = {k: torch.from_numpy(v).cuda() for k, v in AC.make_noise(name, seed=seed).items()}
    wm_noise = dict(q_prior=n["q_prior"].contiguous(), q_post=n["q_post"].contiguous())
    im_noise = dict(act=Hh.to_time_major_rows(n["act"], B, T).contiguous(),
                    q_img=Hh.to_time_major_rows(n["q_img"], B, T).contiguous())
    if g is None or AC.gauss(name):
        return wm_noise, im_noise
    pre = "" if tr is None else tr
    wm_noise.update(force_post=onehot_index(g[pre + "post/stoch"]).transpose(0, 1).contiguous().cuda(), flips=flips)
    if prior:
        wm_noise.update(force_prior=onehot_index(g["prior/stoch"]).transpose(0, 1).contiguous().cuda())
    st = onehot_index(g[pre + "imag/stoch"] if imag_stoch is None else imag_stoch)  # [H,N,S], state t; rows b*T+t
    st = Hh.to_time_major_rows(st, B, T)
    f_img = torch.zeros_like(st)
    f_img[:-1] = st[1:]  # the draw of step t yields state t+1
    im_noise.update(force_img=f_img.contiguous().cuda(), flips=flips)
    if s["actor_dist"] == "onehot":
        act = g[pre + "imag/action"] if imag_action is None else imag_action
        im_noise.update(force_act=Hh.to_time_major_rows(onehot_index(act), B, T).contiguous().cuda())
    return wm_noise, im_noise


def build_p2e(name, wm, cfg):
    """exploration.Plan2Explore with common.make_p2e_weights loaded (tests/test_autograd_gpu.py::_build_p2e)."""
    import exploration

    extr = lambda f, st, a: wm.heads["reward"](f).mean()  # dreamer.py:80
    p2e = exploration.Plan2Explore(cfg, wm, extr).cuda()
    sd = p2e.state_dict()
    for k, v in common.make_p2e_weights(name).items():
        assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
        sd[k] = torch.from_numpy(v)
        if k.startswith("_behavior.actor."):
            sd[k[len("_behavior."):]] = sd[k]  # exploration.py:47: the same module under a second name
    p2e.load_state_dict(sd)
    p2e.requires_grad_(False)
    return p2e
