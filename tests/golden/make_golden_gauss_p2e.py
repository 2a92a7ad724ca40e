#!/usr/bin/env python3
"""Golden vectors of Plan2Explore on continuous latents (dyn_discrete: 0), from the REFERENCE itself (build container
only; the .npz files written here are data and travel, the reference does not).

    python tests/golden/make_golden_gauss_p2e.py [--only NAME]     # writes tests/golden/tiny_gauss_p2e{,_ac}.npz

make_golden.run_p2e at the shapes of make_golden_gauss.py: the reference import, its config loader, the noise tape
and the hooks that replace its random draws are make_golden.py's, the world model with gauss_common's weights is
built by make_golden_gauss.build_reference (both imported read-only), and every N(0,1) draw of the reference -- the
prior's and the posterior's in observe, the actor's and the prior's in imagination -- comes from the recorded tape.
As there, torch.nn.functional.softplus is bound to the missing `torch.softplus` while the generator runs.

One exploration update of the reference's exploration.Plan2Explore after the world model's own update, ordered as
dreamer.py:194-203: wm._train(data) -> p2e.train(start, context, data).  The configurations and the layout of what
is stored are gauss_p2e_common's (P2E, fixture_layout)."""
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

from tests.golden import gauss_common as GC, gauss_p2e_common as GP  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden import make_golden_gauss as MGG  # noqa: E402
from tests.golden.make_golden import Tape  # noqa: E402


def run_p2e(name, models):
    sys.path.insert(0, MG.REF)
    import exploration

    cfg, wm, beh, w = MGG.build_reference(GP.BASE, models)
    for k, v in dict(GP.P2E[name], expl_behavior="plan2explore").items():
        setattr(cfg, k, v)
    extr = lambda f, st, a: wm.heads["reward"](f).mean()  # dreamer.py:80
    with contextlib.redirect_stdout(io.StringIO()):
        p2e = exploration.Plan2Explore(cfg, wm, extr)
    p2e.requires_grad_(False)
    pw = GP.make_p2e_weights(name)
    sd = p2e.state_dict()
    # (`actor.*` are aliases of `_behavior.actor.*`: exploration.py:47 registers the same module twice)
    own = {k for k in sd if not k.startswith(("_behavior._world_model.", "actor.")) and k != "_behavior.ema_vals"}
    assert own == set(pw), own ^ set(pw)
    for k in own:
        assert tuple(sd[k].shape) == pw[k].shape, (k, sd[k].shape, pw[k].shape)
        sd[k] = torch.from_numpy(pw[k])
        if k.startswith("_behavior.actor."):
            sd[k[len("_behavior."):]] = sd[k]
    p2e.load_state_dict(sd)
    data = GC.make_batch(name)
    noise = GC.make_noise(name)
    noise_x = GC.make_noise(name, seed=GP.NOISE_SEED_X)
    out = {}
    quiet = contextlib.redirect_stdout(io.StringIO())

    # gradients as the optimizers see them (after clipping, which is inactive at these norms), caught at Adam.step
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

    MG.TAPE = Tape(GC.observe_tape(noise))
    with quiet:
        post, context, _ = wm._train({k: v.copy() for k, v in data.items()})
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    assert set(post) == {"stoch", "deter", "mean", "std"}, set(post)
    MG.TAPE = Tape(GC.imagine_tape(noise_x))
    with quiet:
        _, mets = p2e.train(post, context, {k: v.copy() for k, v in data.items()})
    assert MG.TAPE.pos == len(MG.TAPE.arrays)
    MG.TAPE = None
    for k in GP.TRAIN_KEYS:
        out["train/" + k] = np.asarray(mets[k], np.float64)
    out["imag/reward"] = MGG.to_np(seen["reward"])
    out["imag/feat"] = MGG.to_np(seen["feat"])
    out["imag/action"] = MGG.to_np(seen["action"])
    for k, g in grabbed.items():
        out["grad/" + k] = MGG.to_np(g)
    for k, v in p2e.state_dict().items():
        if not k.startswith(("_behavior._world_model.", "actor.")):
            out["after/" + k] = MGG.to_np(v)
    out["post/stoch"], out["post/deter"] = MGG.to_np(post["stoch"]), MGG.to_np(post["deter"])
    out["meta/name"] = np.array(name)
    lay = GP.fixture_layout(name)
    assert set(out) == set(lay), set(out) ^ set(lay)
    for k, shp in lay.items():
        assert k == "meta/name" or tuple(out[k].shape) == shp, (k, out[k].shape, shp)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays; explorer_loss="
          f"{float(out['train/explorer_loss']):.6f} actor_loss={float(out['train/actor_loss']):.6f} "
          f"reward mean {float(out['imag/reward'].mean()):.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    tools, networks, models = MG.import_reference()
    MG.install_noise_hooks(tools)
    if not hasattr(torch, "softplus"):
        torch.softplus = torch.nn.functional.softplus
    for name in GP.NAMES:
        if args.only in (None, name):
            run_p2e(name, models)


if __name__ == "__main__":
    main()
