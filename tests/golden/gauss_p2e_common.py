"""Plan2Explore on continuous latents (dyn_discrete: 0): the two fixture configurations, the explorer's deterministic
weights and the declared layout of the fixtures, shared by their generator (make_golden_gauss_p2e.py) and the tests.

Nothing here imports the reference.  The configurations are the `tiny_gauss` world model with the Plan2Explore
settings of `tiny_p2e` / `tiny_p2e_ac`; the action-conditioned one predicts `feat` = [stoch | deter], the one
disag_target that is well-formed only when the state is not one-hot expanded (exploration.py:54-59 sizes it as
dyn_stoch + dyn_deter).  Importing this module adds them to the shape table (dv3hip.shapes.SHAPES, the table
common / gauss_common / helpers read) under their fixture names; world-model weights, batches and noise are
gauss_common's for `tiny_gauss` (they depend on the shapes only)."""
from __future__ import annotations

import zlib
from typing import Dict, Tuple

import numpy as np

from tests.golden import gauss_common as GC
from tests.golden.common import SHAPES

BASE = "tiny_gauss"
P2E = {
    "tiny_gauss_p2e": dict(disag_models=3, disag_layers=2, disag_units=16, disag_target="stoch", disag_offset=1,
                           disag_log=True, disag_action_cond=False, expl_intr_scale=1.0, expl_extr_scale=0.0),
    "tiny_gauss_p2e_ac": dict(disag_models=4, disag_layers=3, disag_units=24, disag_target="feat", disag_offset=1,
                              disag_log=False, disag_action_cond=True, expl_intr_scale=0.7, expl_extr_scale=0.5),
}
NAMES = tuple(P2E)
for _name, _p2e in P2E.items():
    SHAPES.setdefault(_name, dict(SHAPES[BASE], p2e=dict(_p2e)))

TRAIN_KEYS = ("explorer_loss", "explorer_grad_norm", "actor_loss", "actor_grad_norm", "value_loss", "value_grad_norm",
              "actor_entropy", "EMA_005", "EMA_095", "imag_reward_mean", "imag_reward_std", "target_mean", "value_mean")
NOISE_SEED_X = 5  # the exploration behaviour's own imagination draws (as make_golden.run_p2e)


def target_width(name: str, target: str = None) -> int:
    s = SHAPES[name]
    return {"stoch": s["stoch"], "deter": s["deter"], "embed": s["cnn_depth"] * 8 * 16,
            "feat": s["stoch"] + s["deter"]}[target or s["p2e"]["disag_target"]]


def make_weights(name: str) -> Dict[str, np.ndarray]:
    """World model + task behaviour: gauss_common's `tiny_gauss` weights."""
    return GC.make_weights(BASE)


def p2e_param_shapes(name: str) -> Dict[str, Tuple[int, ...]]:
    """common.p2e_param_shapes for `stoch` wide states (and the `feat` target)."""
    s = SHAPES[name]
    c = s["p2e"]
    inp = s["stoch"] + s["deter"] + (s["A"] if c["disag_action_cond"] else 0)
    out, U = target_width(name), c["disag_units"]
    sh: Dict[str, Tuple[int, ...]] = {}
    for i in range(c["disag_models"]):
        for j in range(c["disag_layers"]):
            sh[f"_networks.{i}.layers.NoName_linear{j}.weight"] = (U, inp if j == 0 else U)
            sh[f"_networks.{i}.layers.NoName_norm{j}.weight"] = (U,)
            sh[f"_networks.{i}.layers.NoName_norm{j}.bias"] = (U,)
        sh[f"_networks.{i}.mean_layer.weight"] = (out, U)
        sh[f"_networks.{i}.mean_layer.bias"] = (out,)
    for k, v in GC.param_shapes(BASE).items():
        if k.split(".")[0] in ("actor", "value", "_slow_value"):
            sh["_behavior." + k] = v
    return sh


def make_p2e_weights(name: str, seed: int = 3) -> Dict[str, np.ndarray]:
    """The scheme of common.make_p2e_weights (its own seed: the exploration actor / critic differ from the task's)."""
    out = {}
    for k, shp in p2e_param_shapes(name).items():
        rs = np.random.RandomState((zlib.crc32(k.encode()) + 7919 * seed) & 0x7FFFFFFF)
        if len(shp) == 1:
            w = (1.0 + 0.1 * rs.randn(*shp)) if k.endswith(".weight") and "norm" in k else 0.1 * rs.randn(*shp)
        else:
            w = rs.randn(*shp) * np.sqrt(2.0 / (shp[0] + shp[1]))
            if "value" in k and "mean_layer" in k:
                w *= 0.3
        out[k] = w.astype(np.float32)
    return out


def fixture_layout(name: str) -> Dict[str, Tuple[int, ...]]:
    """{array name: shape} of tests/golden/<name>.npz -- what the generator writes and the tests read:
    train/*      the metric dict of Plan2Explore.train (scalars);
    imag/*       the intrinsic reward [H, N, 1] on the imagined feat [H, N, S + De] / action [H, N, A] (rows b * T + t);
    grad/*       the gradients the three optimizers step on (the members', the exploration actor's and critic's);
    after/*      every parameter (and the return-normalisation EMA) of the module after the update;
    post/*       the posterior the update started from."""
    s = SHAPES[name]
    B, T, H, S, De, A = s["B"], s["T"], s["H"], s["stoch"], s["deter"], s["A"]
    N = B * T
    lay: Dict[str, Tuple[int, ...]] = {"train/" + k: () for k in TRAIN_KEYS}
    lay.update({"imag/reward": (H, N, 1), "imag/feat": (H, N, S + De), "imag/action": (H, N, A),
                "post/stoch": (B, T, S), "post/deter": (B, T, De), "meta/name": ()})
    for k, shp in p2e_param_shapes(name).items():
        lay["after/" + k] = shp
        if not k.startswith("_behavior._slow_value."):
            lay["grad/" + k] = shp
    lay["after/_behavior.ema_vals"] = (2,)
    return lay
