"""`exploration` module with the reference's surface (exploration.py:10-135): `Random` and `Plan2Explore`.

Plan2Explore trains an ensemble of one-step predictors on the replay batch and uses their disagreement on imagined
states as the reward of a second ImagBehavior.  It is written against the PUBLIC surface of this package only --
`networks.MLP(...)(inputs).log_prob / .mode`, `tools.Optimizer(...)(loss, params)`, `ImagBehavior._train(start,
objective)` -- exactly the calls the reference's own exploration.py makes, so either file drives the accelerated
modules: the ensemble runs on the HIP kernels forward and backward through dv3hip.autograd, and the intrinsic reward
enters the hand-written reverse imagination rollout through `ImagBehavior.train_fwd_bwd`'s objective hook.
State-dict keys (`_networks.<i>.layers...`, `_behavior.*`) are the reference's.

Beside that public-surface `train`, `train_fwd_bwd` + `train_opt` run the same update without torch autograd: the
ensemble on the member-batched kernels (dv3hip.engine.EnsembleEngine: one launch per layer for all members) and the
intrinsic reward as ImagBehavior's "ensemble disagreement" objective (models.EnsembleObjective).
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch
from torch import distributions as torchd
from torch import nn

import models
import networks
import tools


class Random(nn.Module):
    """Uniform random policy (exploration.py:10-37): `actor(feat)` ignores feat and returns a distribution over one
    action per environment; `train` is a no-op."""

    def __init__(self, config, act_space):
        super().__init__()
        self._config, self._act_space = config, act_space

    def actor(self, feat):
        cfg = self._config
        if cfg.actor["dist"] == "onehot":
            return tools.OneHotDist(torch.zeros(cfg.envs, cfg.num_actions, device=cfg.device))
        bound = lambda b: torch.as_tensor(np.asarray(b), dtype=torch.float32, device=cfg.device).repeat(cfg.envs, 1)
        return torchd.independent.Independent(
            torchd.uniform.Uniform(bound(self._act_space.low), bound(self._act_space.high)), 1)

    def train(self, start, context, data):
        return None, {}


class Plan2Explore(nn.Module):
    def __init__(self, config, world_model, reward):
        super().__init__()
        if config.precision != 32:
            raise NotImplementedError("the path is fp32 (configs.yaml:18)")
        self._config, self._reward = config, reward
        self._behavior = models.ImagBehavior(config, world_model)
        self.actor = self._behavior.actor
        flat_stoch = config.dyn_stoch * (config.dyn_discrete or 1)
        feat_size = flat_stoch + config.dyn_deter
        # width of what the ensemble predicts; "feat" keeps the reference's (un-flattened) size, exploration.py:58-63
        target_size = dict(embed=world_model.embed_size, stoch=flat_stoch, deter=config.dyn_deter,
                           feat=config.dyn_stoch + config.dyn_deter)[config.disag_target]
        in_size = feat_size + (config.num_actions if config.disag_action_cond else 0)
        self._networks = nn.ModuleList(
            networks.MLP(inp_dim=in_size, shape=target_size, layers=config.disag_layers, units=config.disag_units,
                         act=config.act, device=config.device)
            for _ in range(config.disag_models))
        # members= (fused path only; expl_fused False keeps the flat layout as it was): the bucket lays the members'
        # copies of each parameter side by side (one strided tensor per layer for the member-batched kernels);
        # parameter order, optimizer state and state_dict keys are unchanged
        self._expl_opt = tools.Optimizer("explorer", self._networks.parameters(), config.model_lr, config.opt_eps,
                                         config.grad_clip, wd=config.weight_decay, opt=config.opt, use_amp=False,
                                         members=config.disag_models if self._wants_fused() else 0)
        self._told = False

    # -- the fused path -----------------------------------------------------------------------------------------
    def _wants_fused(self) -> bool:
        cfg = self._config
        return (bool(getattr(cfg, "expl_fused", True)) and bool(getattr(cfg, "norm", True)) and cfg.disag_models >= 2
                and cfg.disag_layers >= 1 and cfg.disag_units <= 2048)

    def fused_reason(self):
        """None when train_fwd_bwd / train_opt can run this configuration, else why not (then `train` is the path)."""
        cfg = self._config
        if not bool(getattr(cfg, "expl_fused", True)):
            return "expl_fused is off"
        if not bool(getattr(cfg, "norm", True)):
            return "norm is False (the fused explorer update is built for the LayerNorm layers)"
        if cfg.disag_models < 2 or cfg.disag_layers < 1 or cfg.disag_units > 2048:
            return "ensemble shape (needs >= 2 members, >= 1 layer, <= 2048 units)"
        if self._expl_opt.bucket.members < 2:
            return "the module was built with expl_fused off (flat explorer bucket)"
        return None

    def fused(self) -> bool:
        why = self.fused_reason()
        if why is not None and not self._told and bool(getattr(self._config, "expl_fused", True)):
            print(f"[dv3hip] Plan2Explore: {why}; the explorer takes the autograd route", file=sys.stderr)
            self._told = True
        return why is None

    def _ensemble(self):
        """(EnsembleEngine over the explorer bucket, the objective marker handed to the behaviour)."""
        import networks as N_
        from dv3hip import engine as E

        cfg = self._config
        dev = next(self._networks.parameters()).device
        ens = self.__dict__.get("_ens")
        if ens is None or ens[0].ws.device != dev:
            head = self._networks[0]
            # the fixed std of networks.MLP's Normal head (networks.py:614, 693-696)
            std = (head._max_std - head._min_std) / (1.0 + math.exp(-(float(head._std) + 2.0))) + head._min_std
            eng = E.EnsembleEngine("p2e", self._expl_opt.bucket, cfg.disag_layers, N_._workspace(self, dev), std=std,
                                   scale=cfg.expl_intr_scale, log=cfg.disag_log, act=head._act_code)
            ens = (eng, models.EnsembleObjective(eng, cfg.disag_action_cond, cfg.expl_extr_scale))
            self.__dict__["_ens"] = ens
        return ens

    def train_fwd_bwd(self, start, context, data, noise=None, allreduce=True):
        """`train` without autograd, first half: the ensemble's regression forward / backward AND its Adam step (the
        behaviour must see the updated members, as in `train`), then the exploration behaviour's forward / backward
        on their disagreement.  noise: as ImagBehavior.train_fwd_bwd.  The two stages are callable one by one
        (train_regress, train_behave): graph.UpdateRunner captures them as separate segments with the explorer
        bucket's all-reduce between them."""
        self.train_regress(start, context, data)
        self.train_behave(start, noise, allreduce)

    def train_regress(self, start, context, data):
        """Ensemble regression on the replay batch: forward, loss, gradients into the explorer bucket."""
        why = self.fused_reason()
        if why is not None:
            raise NotImplementedError(f"Plan2Explore.train_fwd_bwd: {why}")
        cfg = self._config
        if not cfg.dyn_discrete:
            return self._regress_gauss(start, context, data)
        eng, _ = self._ensemble()
        stoch = start["stoch"]
        stoch = stoch.reshape(tuple(stoch.shape[:-2]) + (stoch.shape[-2] * stoch.shape[-1],))
        deter, off = start["deter"], cfg.disag_offset
        # (feat = [stoch | deter], networks.py:154-159, assembled here: `context` caches what it computes lazily, and a
        # replayed launch sequence must not depend on whether somebody has read context["feat"] before)
        target = dict(embed=lambda: context["embed"], stoch=lambda: stoch, deter=lambda: deter,
                      feat=lambda: torch.cat([stoch, deter], -1))[cfg.disag_target]()
        B, T = deter.shape[0], deter.shape[1] - off
        SD, F_ = stoch.shape[-1], stoch.shape[-1] + deter.shape[-1]
        A = cfg.num_actions if cfg.disag_action_cond else 0
        ws = eng.ws
        x = ws.get("p2e.x", (B, T, F_ + A))
        x[..., :SD].copy_(stoch[:, :T])
        x[..., SD:F_].copy_(deter[:, :T])
        if A:
            act = data["action"]
            act = act if isinstance(act, torch.Tensor) else torch.as_tensor(np.asarray(act))
            x[..., F_:].copy_(act.to(x.device, torch.float32)[:, :T])
        tg = ws.get("p2e.target", (B, T, target.shape[-1]))
        tg.copy_(target[:, off:])
        self._expl_opt.begin()
        self._loss = eng.regress_fwd_bwd(x.view(B * T, -1), tg.view(B * T, -1))

    def _regress_gauss(self, start, context, data):
        """train_regress for continuous latents (dyn_discrete: 0): stoch is [B, T, S] (nothing to flatten), the input
        is [stoch | deter | action?] and every disag_target is well-formed (feat = [stoch | deter], S + De wide:
        exploration.py:54-59).  Input and target are assembled by ops.ens_pack_rows, one launch each, with the rows in
        TIME-major order (t * B + b): the posterior of WorldModel._train is a [B, T] view of time-major storage, so
        its steps [0, T - off) and [off, T) are row ranges of one 2-D matrix.  The regression is a mean over the rows;
        their order is free."""
        from dv3hip import ops

        cfg = self._config
        eng, _ = self._ensemble()
        off = cfg.disag_offset

        def tm(v):  # [B, T, W] -> contiguous [T, B, W]; no copy for the world model's own time-major tensors
            v = v.transpose(0, 1)
            return v if v.is_contiguous() else v.contiguous()

        stoch, deter = tm(start["stoch"]), tm(start["deter"])
        Tall, B = deter.shape[0], deter.shape[1]
        T = Tall - off
        S, De = stoch.shape[-1], deter.shape[-1]
        A = cfg.num_actions if cfg.disag_action_cond else 0
        ws = eng.ws
        rows = lambda v, lo, hi: v[lo:hi].reshape((hi - lo) * B, v.shape[-1])
        act = None
        if A:
            act = data["action"]
            act = act if isinstance(act, torch.Tensor) else torch.as_tensor(np.asarray(act))
            act = ops.transpose01(act.to(stoch.device, torch.float32).contiguous(), ws.get("p2e.act_tm", (Tall, B, A)))
        x = ws.get("p2e.x", (T * B, S + De + A))
        ops.ens_pack_rows(x, rows(stoch, 0, T), rows(deter, 0, T), rows(act, 0, T) if A else None)
        # (feat from the posterior, not context["feat"]: `context` caches what it computes lazily, and a replayed
        # launch sequence must not depend on whether somebody has read it before)
        parts = dict(embed=lambda: (tm(context["embed"]),), stoch=lambda: (stoch,), deter=lambda: (deter,),
                     feat=lambda: (stoch, deter))[cfg.disag_target]()
        tg = ws.get("p2e.target", (T * B, sum(p.shape[-1] for p in parts)))
        ops.ens_pack_rows(tg, *[rows(p, off, Tall) for p in parts])
        self._expl_opt.begin()
        self._loss = eng.regress_fwd_bwd(x, tg)

    def train_behave(self, start, noise=None, allreduce=True):
        """The ensemble's clip + Adam step, then the exploration behaviour's forward / backward on the updated
        members' disagreement.  allreduce=False: the caller has all-reduced the explorer bucket."""
        # (snapshots: the loss lives in a workspace buffer, the norm in the bucket's state vector)
        self._pending = {k: v.detach().clone() for k, v in self._expl_opt.finish(self._loss, allreduce).items()}
        self._behavior.train_fwd_bwd(start, noise, self._ensemble()[1])

    def train_opt(self, allreduce=True):
        """Second half: the exploration actor's and critic's optimizer steps -> (None, metrics of `train`)."""
        metrics = dict(self._pending)
        metrics.update(self._behavior.train_opt(allreduce)[-1])
        return None, metrics

    # -- one exploration update: ensemble regression on the replay batch, then the behaviour on its disagreement ----
    def train(self, start, context, data):
        cfg = self._config
        stoch = start["stoch"]
        if cfg.dyn_discrete:
            stoch = stoch.reshape(tuple(stoch.shape[:-2]) + (stoch.shape[-2] * stoch.shape[-1],))
        pick = dict(embed=lambda: context["embed"], stoch=lambda: stoch, deter=lambda: start["deter"],
                    feat=lambda: context["feat"])
        target = pick[cfg.disag_target]()
        inputs = context["feat"]
        if cfg.disag_action_cond:
            act = data["action"]
            act = act if isinstance(act, torch.Tensor) else torch.as_tensor(np.asarray(act))
            inputs = torch.cat([inputs, act.to(inputs.device, torch.float32)], -1)
        metrics = {}
        with tools.RequiresGrad(self._networks):
            metrics.update(self._train_ensemble(inputs, target))
        metrics.update(self._behavior._train(start, self._intrinsic_reward)[-1])
        return None, metrics

    def _train_ensemble(self, inputs, targets):
        """Each member maximises the likelihood of the (offset) target under its Normal head; one Adam step on the
        mean over members (exploration.py:123-135)."""
        off = self._config.disag_offset
        if off:
            targets, inputs = targets[:, off:], inputs[:, :-off]
        targets, inputs = targets.detach(), inputs.detach()
        like = torch.stack([head(inputs).log_prob(targets).mean() for head in self._networks])
        return self._expl_opt(-like.mean(), self._networks.parameters())

    def _intrinsic_reward(self, feat, state, action):
        """Disagreement = std over the members' predictions, averaged over the target dimensions (log'd with
        disag_log), scaled; plus the scaled extrinsic reward if configured (exploration.py:108-121)."""
        cfg = self._config
        x = torch.cat([feat, action], -1) if cfg.disag_action_cond else feat
        preds = torch.stack([head(x, torch.float32).mode() for head in self._networks], 0)
        disag = preds.std(0).mean(-1, keepdim=True)
        if cfg.disag_log:
            disag = disag.log()
        reward = cfg.expl_intr_scale * disag
        if cfg.expl_extr_scale:
            reward = reward + cfg.expl_extr_scale * self._reward(feat, state, action)
        return reward
