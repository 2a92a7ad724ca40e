#!/usr/bin/env python3
"""Golden vectors of the LayerNorm-free configurations (norm / encoder.norm / decoder.norm: False), from the REFERENCE
itself (build container only; the files written here are data and travel, the reference does not).

    python tests/golden/make_golden_nonorm.py [--only NAME]
        # writes tests/golden/tiny_nonorm.npz, tiny_nonorm_video.npz, tiny_nonorm_mix.npz and nonorm_surface.json

The run itself is make_golden_act.py's (run_config / run_video: the world model's and the behaviour's outputs, every
gradient, two consecutive updates through the reference's own `_train` pair, three acting steps on two environments),
with nonorm_common's tables in place of act_common's and the shapes' `norm` / `enc_norm` / `dec_norm` keys as the
reference's config keys `norm` / `encoder.norm` / `decoder.norm`.

Asserted while generating:
  * the reference's state_dict key set equals nonorm_common.param_shapes (names and shapes);
  * no module of a group whose key is False is a LayerNorm, every group whose key is True still has one;
  * the GRU pre-activations (the output of GRU_linear) of the whole run stay within +-nonorm_common.GRU_PRE_MAX; the
    observed maximum is stored as meta/gru_pre_absmax.

nonorm_surface.json: for each of the 8 combinations of the three keys on the tiny_mixed row, the names and shapes of
the reference's WorldModel + ImagBehavior state_dict.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import common  # noqa: E402
from tests.golden import make_golden_act as MA  # noqa: E402
from tests.golden import nonorm_common as NC  # noqa: E402
from tests.golden.make_golden import ObsSpace, Space, import_reference, install_noise_hooks, load_config  # noqa: E402

GRU_ABSMAX = [0.0]


def _gru_hook(mod, inp, out):
    GRU_ABSMAX[0] = max(GRU_ABSMAX[0], float(out.detach().abs().max()))


def reference_models(s, models, norm, enc_norm, dec_norm):
    """The reference's (config, WorldModel, ImagBehavior) for shape row s with the three keys as given."""
    ov = dict(
        device="cpu", compile=False, num_actions=s["A"], dyn_stoch=s["stoch"], dyn_discrete=s["discrete"],
        dyn_deter=s["deter"], dyn_hidden=s["hidden"], units=s["units"], batch_size=s["B"], batch_length=s["T"],
        imag_horizon=s["H"], imag_gradient=s["imag_gradient"], norm=norm,
        encoder=dict(cnn_depth=s["cnn_depth"], norm=enc_norm), decoder=dict(cnn_depth=s["cnn_depth"], norm=dec_norm),
        causal_world_model=False, imag_gradient_mix=0.0, actor=dict(layers=2), critic=dict(layers=2),
        reward_head=dict(layers=2), cont_head=dict(layers=2),
    )
    for key in ("mean_act", "std_act", "min_std"):
        if key in s:
            ov["dyn_" + key] = s[key]
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
    # LayerNorm modules exactly in the groups whose key is True
    has_ln = lambda m: any(isinstance(x, torch.nn.LayerNorm) for x in m.modules())
    groups = {"norm": [wm.dynamics, wm.heads["reward"], wm.heads["cont"], beh.actor, beh.value, beh._slow_value],
              "encoder.norm": [wm.encoder], "decoder.norm": [wm.heads["decoder"]]}
    for (key, mods), on in zip(groups.items(), (norm, enc_norm, dec_norm)):
        for m in mods:
            assert has_ln(m) == bool(on), (key, on, type(m).__name__)
    return cfg, wm, beh


def state_shapes(wm, beh):
    sd = {**dict(wm.state_dict()), **{k: v for k, v in beh.state_dict().items()
                                       if not k.startswith("_world_model.") and k != "ema_vals"}}
    return {k: tuple(v.shape) for k, v in sd.items()}


def build_reference(name, models):
    """make_golden_act.build_reference for the shapes of nonorm_common."""
    s = common.SHAPES[name]
    cfg, wm, beh = reference_models(s, models, *NC.norm_keys(s))
    table = NC.param_shapes(name)
    got = state_shapes(wm, beh)
    assert set(got) == set(table), sorted(set(got) ^ set(table))
    for k, shp in table.items():
        assert got[k] == tuple(shp), (k, got[k], shp)
    wm.dynamics._cell.layers.GRU_linear.register_forward_hook(_gru_hook)
    wm.requires_grad_(False)
    beh.requires_grad_(False)
    w = NC.make_weights(name)
    wm.load_state_dict({k: torch.from_numpy(v) for k, v in w.items() if k.split(".")[0] in ("encoder", "dynamics", "heads")})
    sd_beh = beh.state_dict()
    for k in sd_beh:
        if not k.startswith("_world_model.") and k != "ema_vals":
            sd_beh[k] = torch.from_numpy(w[k])
    beh.load_state_dict(sd_beh)
    return cfg, wm, beh, w


def write_surface(models):
    s = common.SHAPES[NC.SURFACE_ROW]
    out = {}
    for (n, e, d), key in NC.surface_combos():
        cfg, wm, beh = reference_models(s, models, n, e, d)
        got = state_shapes(wm, beh)
        table = NC.shapes_of(s, n, e, d)
        assert {k: tuple(v) for k, v in table.items()} == got, (key, sorted(set(got) ^ set(table)))
        out[key] = {k: list(v) for k, v in got.items()}
    path = os.path.join(HERE, "nonorm_surface.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"[golden] wrote {path}: {len(out)} combinations, {os.path.getsize(path) / 1e3:.1f} kB")


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
    MA.AC = NC  # (run_config / run_policy / run_video take their tables and inputs from this module's namesake)
    MA.build_reference = build_reference
    for name in NC.NAMES:
        if args.only not in (None, name):
            continue
        GRU_ABSMAX[0] = 0.0
        out, _ = MA.run_config(name, models)
        del out["meta/relu_min"]
        print(f"[golden] {name}: largest |GRU pre-activation| of the run {GRU_ABSMAX[0]:.3f}")
        assert GRU_ABSMAX[0] <= NC.GRU_PRE_MAX, "lower nonorm_common.GRU_WEIGHT_SCALE: the GRU gates saturate"
        out["meta/gru_pre_absmax"] = np.float64(GRU_ABSMAX[0])
        out["meta/norm_keys"] = np.array(NC.norm_keys(common.SHAPES[name]))
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"[golden] wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays; "
              f"model_loss={float(out['model_loss']):.6f} actor_loss={float(out['actor_loss']):.6f} "
              f"value_loss={float(out['value_loss']):.6f}")
    if args.only in (None, NC.VIDEO + "_video"):
        MA.run_video(NC.VIDEO, models)
    if args.only in (None, "surface"):
        write_surface(models)


if __name__ == "__main__":
    main()
