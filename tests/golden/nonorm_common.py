"""Deterministic inputs of the LayerNorm-free fixtures (config keys norm / encoder.norm / decoder.norm: False), shared
by their generator (make_golden_nonorm.py) and the tests.  Nothing here imports the reference.

The shapes live in dv3hip.shapes.SHAPES (tiny_nonorm, tiny_nonorm_mix).  The parameter table of a shape is that of
common.param_shapes / gauss_common.param_shapes with the LayerNorm entries of the keys that are False dropped and the
conv nn.Sequentials renumbered, as the reference builds the modules (networks.py:53-78, 465-477, 528-554, 627-633,
751-754):

  norm False          dynamics._img_in_layers.1.*, ._img_out_layers.1.*, ._obs_out_layers.1.*, ._cell.layers.GRU_norm.*
                      and every <Name>_norm<i> of the reward / cont heads, the actor and both critics disappear
  encoder.norm False  encoder._cnn.layers.{3i} -> {2i} (the {3i+1}.norm entries disappear); encoder._mlp Encoder_norm<i>
  decoder.norm False  heads.decoder._cnn.layers.{0,3,6,9} -> {0,2,4,6}; heads.decoder._mlp Decoder_norm<i>

Batches, update noise and acting-step inputs are those of common (categorical latents) or gauss_common (dyn_discrete:
0) under the shape's name."""
from __future__ import annotations

import re
import zlib
from typing import Dict, Tuple

import numpy as np

from tests.golden import common, gauss_common as GC
from tests.golden.common import PROPRIO_KEYS, SHAPES

NAMES = ("tiny_nonorm", "tiny_nonorm_mix")
VIDEO = "tiny_nonorm"
SURFACE_ROW = "tiny_mixed"  # nonorm_surface.json: the 8 combinations of the three keys on this row
POLICY_ENVS, POLICY_STEPS = GC.POLICY_ENVS, GC.POLICY_STEPS
# Weight scale of the GRU's Linear.  make_golden_nonorm.py asserts that the GRU pre-activations of the whole reference
# run stay within +-GRU_PRE_MAX (past that the gates saturate and a comparison shows nothing) and this constant is to
# be lowered if they do not.  At 1.0 (the scale of common.make_weights) the observed maxima are far inside the range
# (the fixtures' meta/gru_pre_absmax).
GRU_WEIGHT_SCALE = 1.0
GRU_PRE_MAX = 10.0
# both stat layers' scale of the Gaussian shape (as gauss_common.STAT_SCALE)
STAT_SCALE = {"tiny_nonorm_mix": 0.5}
WEIGHT_SEED: Dict[str, int] = {}
RELU_MARGIN = 1e-4  # (no shape here has a ReLU; make_golden_act.run_config reads the name)
P2E = None


def gauss(name: str) -> bool:
    return not SHAPES[name]["discrete"]


def src(name: str):
    """The module whose make_noise / tapes fit the shape's latent kind."""
    return GC if gauss(name) else common


def state_keys(name: str):
    return ("stoch", "deter", "mean", "std") if gauss(name) else ("stoch", "deter", "logit")


def norm_keys(s) -> Tuple[bool, bool, bool]:
    """(norm, encoder.norm, decoder.norm) of a shape row."""
    return bool(s.get("norm", True)), bool(s.get("enc_norm", True)), bool(s.get("dec_norm", True))


def _base_shapes(s) -> Dict[str, Tuple[int, ...]]:
    """The norm: True table of shape row s by reference state_dict name."""
    tmp = "#nonorm_common"
    if s["discrete"]:
        SHAPES[tmp] = dict(s)
    else:
        # continuous latents: common's table at discrete = 1 has every width right (the state is `stoch` wide) but the
        # stat layers', which are 2 * stoch (mean_raw | std_raw); gauss_common's own table has no vector observations
        SHAPES[tmp] = dict(s, discrete=1)
    try:
        sh = dict(common.param_shapes(tmp))
    finally:
        del SHAPES[tmp]
    if not s["discrete"]:
        for nm in ("_imgs_stat_layer", "_obs_stat_layer"):
            sh[f"dynamics.{nm}.weight"] = (2 * s["stoch"], s["hidden"])
            sh[f"dynamics.{nm}.bias"] = (2 * s["stoch"],)
    return sh


_TRUNK_NORM = re.compile(r"^(heads\.reward|heads\.cont|actor|value|_slow_value)\.layers\.\w+_norm\d+\.")
_RSSM_NORM = re.compile(r"^dynamics\.(_img_in_layers\.1|_img_out_layers\.1|_obs_out_layers\.1|_cell\.layers\.GRU_norm)\.")


def shapes_of(s, norm=None, enc_norm=None, dec_norm=None) -> Dict[str, Tuple[int, ...]]:
    """Parameter shapes of shape row s with the three keys as given (default: the row's own)."""
    n0, e0, d0 = norm_keys(s)
    norm, enc_norm, dec_norm = (n0 if norm is None else norm, e0 if enc_norm is None else enc_norm,
                                d0 if dec_norm is None else dec_norm)
    out: Dict[str, Tuple[int, ...]] = {}
    for k, shp in _base_shapes(s).items():
        if not norm and (_RSSM_NORM.match(k) or _TRUNK_NORM.match(k)):
            continue
        for on, pre, mlp_nm in ((enc_norm, "encoder._cnn.layers.", "encoder._mlp.layers.Encoder_norm"),
                                (dec_norm, "heads.decoder._cnn.layers.", "heads.decoder._mlp.layers.Decoder_norm")):
            if on:
                continue
            if k.startswith(mlp_nm):
                k = None
                break
            if k.startswith(pre):
                idx, rest = k[len(pre):].split(".", 1)
                if int(idx) % 3:  # the ImgChLayerNorm behind conv 3i
                    k = None
                    break
                k = f"{pre}{int(idx) // 3 * 2}.{rest}"
        if k is not None:
            out[k] = shp
    return out


def param_shapes(name: str) -> Dict[str, Tuple[int, ...]]:
    return shapes_of(SHAPES[name])


def make_weights(name: str, seed: int = 0) -> Dict[str, np.ndarray]:
    """One numpy stream per parameter name, scales as common.make_weights / gauss_common.make_weights."""
    out = {}
    for k, shp in param_shapes(name).items():
        rs = np.random.RandomState((zlib.crc32(k.encode()) + 7919 * seed) & 0x7FFFFFFF)
        if k == "dynamics.W":
            w = 0.5 * rs.randn(*shp)
        elif len(shp) == 1:  # (every 1-D ".weight" is a LayerNorm scale)
            w = (1.0 + 0.1 * rs.randn(*shp)) if k.endswith(".weight") else 0.1 * rs.randn(*shp)
        else:
            fan = (shp[0] + shp[1]) * (shp[2] * shp[3] if len(shp) == 4 else 1) / 2.0
            w = rs.randn(*shp) * np.sqrt(1.0 / fan)
            if "mean_layer" in k and ("reward" in k or "value" in k):
                w *= 0.3
            if "_stat_layer" in k and gauss(name):
                w *= STAT_SCALE[name]
            if "GRU_linear" in k:
                w *= GRU_WEIGHT_SCALE
        out[k] = w.astype(np.float32)
    return out


def make_batch(name: str, seed: int = 0):
    return common.make_batch(name, seed=seed)


def make_noise(name: str, seed: int = 0):
    return src(name).make_noise(name, seed=seed)


def make_policy_inputs(name: str, seed: int = 0):
    """act_common.make_policy_inputs for these shapes: POLICY_STEPS acting steps on POLICY_ENVS environments, with the
    vector keys of a shape that has them."""
    if not gauss(name):
        from tests.golden import act_common

        return act_common.make_policy_inputs(name, seed=seed)
    steps = GC.make_policy_inputs(name, seed=seed)
    if SHAPES[name]["encoder"] in ("mlp", "both"):
        rs = np.random.RandomState(7000 + seed)
        for st in steps:
            for k, w in PROPRIO_KEYS:
                st[k] = rs.randn(POLICY_ENVS, w).astype(np.float32)
    return steps


def obs_keys(name: str):
    keys = ["image", "is_first", "is_terminal"]
    if SHAPES[name]["encoder"] in ("mlp", "both"):
        keys += [k for k, _ in PROPRIO_KEYS]
    return keys


def surface_combos():
    """The 8 combinations (norm, encoder.norm, decoder.norm) and their keys in nonorm_surface.json."""
    return [((n, e, d), f"norm={n},encoder.norm={e},decoder.norm={d}") for n in (True, False) for e in (True, False)
            for d in (True, False)]
