"""Deterministic inputs of the continuous-latent (dyn_discrete: 0) fixtures, shared by their generator
(make_golden_gauss.py) and the tests: parameter shapes by reference state_dict name, weights in the style of
common.make_weights, and N(0,1) noise tapes in the order the reference draws them.

Nothing here imports the reference.  common.param_shapes / make_noise assume stoch * discrete wide states; these are
their counterparts for `stoch` wide states with 2 * stoch wide stat layers (image encoder / decoder shapes only).
"""
from __future__ import annotations

import zlib
from typing import Dict, List, Tuple

import numpy as np

from tests.golden.common import SHAPES, make_batch  # noqa: F401  (same table, same synthetic batches)

# Both stat layers' weights are multiplied by this so that the per-step KL values straddle the free-bits floor
# (kl_free = 1): make_golden_gauss.py asserts that at least one stored value is clipped and at least one is not.
STAT_SCALE = {"tiny_gauss": 0.5, "tiny_gauss_onehot": 0.35, "cfg2_gauss": 0.22}
POLICY_ENVS, POLICY_STEPS = 2, 3
SAMPLE = 128  # elements per tensor the full-size fixture keeps of every gradient and Adam-updated parameter


def sample_index(key: str, numel: int) -> np.ndarray:
    """Flat indices of the elements of tensor `key` that the full-size fixture stores (all of a small tensor): a
    function of the name and the size only, so the generator and the tests pick the same elements."""
    if numel <= SAMPLE:
        return np.arange(numel)
    rs = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return np.sort(rs.choice(numel, SAMPLE, replace=False))


def param_shapes(name: str) -> Dict[str, Tuple[int, ...]]:
    s = SHAPES[name]
    assert not s["discrete"] and s["encoder"] == "cnn", name
    S, De, Hd, U, A, d = s["stoch"], s["deter"], s["hidden"], s["units"], s["A"], s["cnn_depth"]
    F, E = S + De, d * 8 * 16
    sh: Dict[str, Tuple[int, ...]] = {}

    def ln(prefix, n):
        sh[prefix + ".weight"] = (n,)
        sh[prefix + ".bias"] = (n,)

    def mlp(prefix, nm, layers, inp, units):
        for i in range(layers):
            sh[f"{prefix}layers.{nm}_linear{i}.weight"] = (units, inp if i == 0 else units)
            ln(f"{prefix}layers.{nm}_norm{i}", units)

    cin = 3
    for i in range(4):
        cout = d * 2**i
        sh[f"encoder._cnn.layers.{3 * i}.weight"] = (cout, cin, 4, 4)
        ln(f"encoder._cnn.layers.{3 * i + 1}.norm", cout)
        cin = cout
    sh["dynamics.W"] = (1, De)
    sh["dynamics._img_in_layers.0.weight"] = (Hd, S + A)
    ln("dynamics._img_in_layers.1", Hd)
    sh["dynamics._cell.layers.GRU_linear.weight"] = (3 * De, Hd + De)
    ln("dynamics._cell.layers.GRU_norm", 3 * De)
    sh["dynamics._img_out_layers.0.weight"] = (Hd, De)
    ln("dynamics._img_out_layers.1", Hd)
    sh["dynamics._obs_out_layers.0.weight"] = (Hd, De + E)
    ln("dynamics._obs_out_layers.1", Hd)
    for nm in ("_imgs_stat_layer", "_obs_stat_layer"):
        sh[f"dynamics.{nm}.weight"] = (2 * S, Hd)
        sh[f"dynamics.{nm}.bias"] = (2 * S,)
    sh["heads.decoder._cnn._linear_layer.weight"] = (E, F)
    sh["heads.decoder._cnn._linear_layer.bias"] = (E,)
    cin = d * 8
    for i in range(3):
        sh[f"heads.decoder._cnn.layers.{3 * i}.weight"] = (cin, cin // 2, 4, 4)
        ln(f"heads.decoder._cnn.layers.{3 * i + 1}.norm", cin // 2)
        cin //= 2
    sh["heads.decoder._cnn.layers.9.weight"] = (cin, 3, 4, 4)
    sh["heads.decoder._cnn.layers.9.bias"] = (3,)
    for pre, nm, out in (("heads.reward.", "Reward", 255), ("heads.cont.", "Cont", 1)):
        mlp(pre, nm, 2, F, U)
        sh[pre + "mean_layer.weight"] = (out, U)
        sh[pre + "mean_layer.bias"] = (out,)
    mlp("actor.", "Actor", 2, F, U)
    sh["actor.mean_layer.weight"] = (A, U)
    sh["actor.mean_layer.bias"] = (A,)
    if s["actor_dist"] == "normal":
        sh["actor.std_layer.weight"] = (A, U)
        sh["actor.std_layer.bias"] = (A,)
    for pre in ("value.", "_slow_value."):
        mlp(pre, "Value", 2, F, U)
        sh[pre + "mean_layer.weight"] = (255, U)
        sh[pre + "mean_layer.bias"] = (255,)
    return sh


def sample_layout(name: str, group: str):
    """{parameter name: (offset, flat indices)} into the full-size fixture's `smp/<group>` array.  group "grad": the
    parameters that receive a gradient (not the slow critic); "after" / "after2": every parameter."""
    sh = dict(param_shapes(name))
    if group != "grad":
        sh["ema_vals"] = (2,)  # (the behaviour's state_dict holds the return-normalisation EMA as well)
    names = sorted(k for k in sh if group != "grad" or not k.startswith("_slow_value."))
    out, off = {}, 0
    for k in names:
        idx = sample_index(k, int(np.prod(sh[k])))
        out[k] = (off, idx)
        off += idx.size
    return out


def delta_names(name: str):
    """Row order of the fixture's `sum/delta/<group>` arrays."""
    return sorted(param_shapes(name))


def make_weights(name: str, seed: int = 0) -> Dict[str, np.ndarray]:
    """One numpy stream per parameter name, scales as common.make_weights; the stat layers times STAT_SCALE."""
    out = {}
    for k, shp in param_shapes(name).items():
        rs = np.random.RandomState((zlib.crc32(k.encode()) + 7919 * seed) & 0x7FFFFFFF)
        if k == "dynamics.W":
            w = 0.5 * rs.randn(*shp)
        elif len(shp) == 1:
            w = (1.0 + 0.1 * rs.randn(*shp)) if k.endswith(".weight") else 0.1 * rs.randn(*shp)
        else:
            fan = (shp[0] + shp[1]) * (shp[2] * shp[3] if len(shp) == 4 else 1) / 2.0
            w = rs.randn(*shp) * np.sqrt(1.0 / fan)
            if "mean_layer" in k and ("reward" in k or "value" in k):
                w *= 0.3
            if "_stat_layer" in k:
                w *= STAT_SCALE[name]
        out[k] = w.astype(np.float32)
    return out


def make_noise(name: str, seed: int = 0) -> Dict[str, np.ndarray]:
    """Every draw of one update: observe q_prior, q_post [T,B,S] ~ N(0,1); imagine act [H,N,A] (N(0,1) for the normal
    actor, Exp(1) for the one-hot actor) and q_img [H,N,S] ~ N(0,1)."""
    s = SHAPES[name]
    B, T, H, S, A = s["B"], s["T"], s["H"], s["stoch"], s["A"]
    N = B * T
    rs = np.random.RandomState(3000 + seed)
    out = {"q_prior": rs.randn(T, B, S).astype(np.float32), "q_post": rs.randn(T, B, S).astype(np.float32),
           "q_img": rs.randn(H, N, S).astype(np.float32)}
    if s["actor_dist"] == "onehot":
        out["act"] = np.maximum(rs.exponential(size=(H, N, A)), 1e-20).astype(np.float32)
    else:
        out["act"] = rs.randn(H, N, A).astype(np.float32)
    return out


def observe_tape(noise) -> List[np.ndarray]:
    """observe draws, per step, the prior's [B,S] then the posterior's [B,S]."""
    tape = []
    for t in range(noise["q_prior"].shape[0]):
        tape += [noise["q_prior"][t], noise["q_post"][t]]
    return tape


def imagine_tape(noise) -> List[np.ndarray]:
    """_imagine draws, per step, the actor's [N,A] then the prior's [N,S]."""
    tape = []
    for t in range(noise["q_img"].shape[0]):
        tape += [noise["act"][t], noise["q_img"][t]]
    return tape


def make_video_noise(name: str, seed: int = 0) -> Dict[str, np.ndarray]:
    s = SHAPES[name]
    bv, T, S = min(6, s["B"]), s["T"], s["stoch"]
    rs = np.random.RandomState(4000 + seed)
    return {"q_prior": rs.randn(5, bv, S).astype(np.float32), "q_post": rs.randn(5, bv, S).astype(np.float32),
            "q_open": rs.randn(T - 5, bv, S).astype(np.float32)}


def video_tape(noise) -> List[np.ndarray]:
    return observe_tape(noise) + [noise["q_open"][t] for t in range(noise["q_open"].shape[0])]


def make_policy_inputs(name: str, seed: int = 0):
    """POLICY_STEPS acting steps on POLICY_ENVS environments: images, is_first (all at step 0 -- the state is None
    there -- and env 1 again at step 1) and the draws prior / post [n,S] ~ N(0,1), act [n,A] of every step."""
    s = SHAPES[name]
    n, S, A = POLICY_ENVS, s["stoch"], s["A"]
    rs = np.random.RandomState(5000 + seed)
    steps = []
    for t in range(POLICY_STEPS):
        first = np.zeros(n, bool)
        if t == 0:
            first[:] = True
        if t == 1:
            first[1] = True
        act = (np.maximum(rs.exponential(size=(n, A)), 1e-20) if s["actor_dist"] == "onehot" else rs.randn(n, A))
        steps.append(dict(image=rs.randint(0, 256, size=(n, 64, 64, 3)).astype(np.uint8), is_first=first,
                          is_terminal=np.zeros(n, bool), prior=rs.randn(n, S).astype(np.float32),
                          post=rs.randn(n, S).astype(np.float32), act=act.astype(np.float32)))
    return steps
