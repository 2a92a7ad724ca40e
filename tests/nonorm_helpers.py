"""Scaffolding of the LayerNorm-free path tests (norm / encoder.norm / decoder.norm: False; fixtures written by
tests/golden/make_golden_nonorm.py from the reference): tests/act_helpers.py's functions over nonorm_common's tables.
The comparisons themselves are tests/gauss_helpers.py's, imported by the tests and not restated here."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import act_helpers as A
from tests import helpers as Hh
from tests.golden import common
from tests.golden import nonorm_common as NC

GOLDEN = A.GOLDEN
WM_METRICS, BEH_METRICS, NORMS = A.WM_METRICS, A.BEH_METRICS, A.NORMS
decoder_keys = A.decoder_keys
onehot_index = A.onehot_index


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def build_models(name, device="cuda:0"):
    return Hh.build_models(name, device, weights=NC.make_weights(name))


def fixture_keys(name):
    """act_helpers.fixture_keys over nonorm_common's parameter table: every key tests/test_nonorm_path_gpu.py reads."""
    sk = NC.state_keys(name)
    keys = ["meta/full", "meta/gru_pre_absmax", "model_loss", "model_grad_norm", "actor_loss", "value_loss",
            "ema_vals_after", "kl_value"]
    keys += [f"{p}/{k}" for p in ("post", "prior", "imag") for k in sk]
    keys += ["imag/action", "imag/feat", "imag/weights", "imag/reward", "imag/target", "imag/value", "imag/actor_ent"]
    for k in NC.param_shapes(name):
        if not k.startswith("_slow_value."):
            keys.append("grad/" + k)
        keys += ["after/" + k, "after2/" + k]
    for tr in ("train/", "train2/"):
        keys += [tr + k for k in ("model_loss",) + WM_METRICS + BEH_METRICS + NORMS]
        keys += [tr + k + "_loss" for k in decoder_keys(name)]
        keys += [tr + "post/stoch", tr + "post/deter", tr + "imag/stoch", tr + "imag/action"]
    tags = ("train", "eval") if NC.gauss(name) else ("train",)
    keys += [f"policy/{tag}/{t}/{k}" for tag in tags for t in range(NC.POLICY_STEPS) for k in sk + ("action", "logprob")]
    return keys


def gpu_noise(name, seed=0, g=None, tr=None, flips=None, prior=True):
    """act_helpers.gpu_noise for nonorm_common's shapes: (wm_noise, im_noise) for WorldModel._train /
    ImagBehavior._train, the categorical draws teacher-forced to the fixture's classes and counted in `flips`."""
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    n = {k: torch.from_numpy(v).cuda() for k, v in NC.make_noise(name, seed=seed).items()}
    wm_noise = dict(q_prior=n["q_prior"].contiguous(), q_post=n["q_post"].contiguous())
    im_noise = dict(act=Hh.to_time_major_rows(n["act"], B, T).contiguous(),
                    q_img=Hh.to_time_major_rows(n["q_img"], B, T).contiguous())
    if g is None or NC.gauss(name):
        return wm_noise, im_noise
    pre = "" if tr is None else tr
    wm_noise.update(force_post=onehot_index(g[pre + "post/stoch"]).transpose(0, 1).contiguous().cuda(), flips=flips)
    if prior:
        wm_noise.update(force_prior=onehot_index(g["prior/stoch"]).transpose(0, 1).contiguous().cuda())
    st = Hh.to_time_major_rows(onehot_index(g[pre + "imag/stoch"]), B, T)  # [H,N,S], state t; rows b*T+t
    f_img = torch.zeros_like(st)
    f_img[:-1] = st[1:]  # the draw of step t yields state t+1
    im_noise.update(force_img=f_img.contiguous().cuda(), flips=flips)
    if s["actor_dist"] == "onehot":
        im_noise.update(force_act=Hh.to_time_major_rows(onehot_index(g[pre + "imag/action"]), B, T).contiguous().cuda())
    return wm_noise, im_noise
