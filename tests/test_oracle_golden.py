"""Pins the CPU oracle (oracle/dv3_oracle.py) to golden vectors produced by the reference.

CPU-only.  Golden .npz files were written by tests/golden/make_golden.py, which runs the
reference's own WorldModel / ImagBehavior with injected sampling noise.
"""
import os

import numpy as np
import pytest
import torch

from oracle import dv3_oracle as O
from tests.golden import common

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WM_PREFIXES = ("encoder", "dynamics", "heads")


def load(name):
    path = os.path.join(GOLD, name + ".npz")
    if not os.path.exists(path):
        pytest.skip(f"{path} missing")
    return np.load(path, allow_pickle=False)


def tparams(name, grad=False):
    p = {k: torch.from_numpy(v.copy()) for k, v in common.make_weights(name).items()}
    if grad:
        for v in p.values():
            v.requires_grad_(True)
    return p


def tnoise(name):
    return {k: torch.from_numpy(v) for k, v in common.make_noise(name).items()}


def _np(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float64)


def close(a, b, tol=2e-5, what=""):
    a = _np(a)
    b = _np(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    scale = max(1.0, np.abs(b).max() if b.size else 1.0)
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e})"


def check_sum(g, key, arr, tol=1e-4):
    ref = g["sum/" + key]
    got = common.checksum(arr)
    assert abs(got[0] - ref[0]) <= tol * max(1.0, ref[1]), (key, got, ref)
    assert abs(got[1] - ref[1]) <= tol * max(1.0, ref[1]), (key, got, ref)


def wm_out(name, grad=False):
    cfg = common.path_config(name)
    p = tparams(name, grad)
    n = tnoise(name)
    data = common.make_batch(name)
    return cfg, p, n, data, O.wm_forward(cfg, p, data, n["q_prior"], n["q_post"])


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_fixture_inputs_regenerate(name):
    """The generator's stored inputs are exactly what common.py regenerates from the seed."""
    g = load(name)
    for k, v in common.make_weights(name).items():
        assert np.array_equal(g["w/" + k], v), k
    for k, v in common.make_batch(name).items():
        assert np.array_equal(g["data/" + k], v), k
    for k, v in common.make_noise(name).items():
        assert np.array_equal(g["noise/" + k], v), k


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_world_model_forward_full(name):
    g = load(name)
    cfg, p, n, data, out = wm_out(name)
    close(out["embed"], g["embed"], what="embed")
    for k in ("stoch", "deter", "logit"):
        close(out["post"][k], g["post/" + k], what="post/" + k)
        close(out["prior"][k], g["prior/" + k], what="prior/" + k)
    # sampled one-hots must agree exactly (no flips at this size on the same host)
    assert np.array_equal(out["post"]["stoch"].detach().numpy(), g["post/stoch"])
    if cfg.encoder in ("cnn", "both"):
        close(out["recon"], g["recon"], what="recon")
    if cfg.encoder in ("mlp", "both"):
        for k, _ in cfg.mlp_keys:  # (the vector decoder's per-key modes, in symlog space)
            close(out["recon_modes"][k], g["recon/" + k], what="recon/" + k)
    close(out["reward_logits"], g["reward_logits"], what="reward_logits")
    close(out["cont_logit"], g["cont_logit"], what="cont_logit")
    for k, v in out["losses"].items():
        close(v, g["loss/" + k], tol=1e-5, what="loss/" + k)
    close(out["kl"], g["kl_value"], what="kl")
    close(out["dyn_loss"], g["dyn_loss"], what="dyn")
    close(out["rep_loss"], g["rep_loss"], what="rep")
    close(out["prior_ent"], g["prior_ent"], what="prior_ent")
    close(out["post_ent"], g["post_ent"], what="post_ent")
    close(out["model_loss"], g["model_loss"], tol=1e-6, what="model_loss")


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_world_model_gradients(name):
    g = load(name)
    cfg, p, n, data, out = wm_out(name, grad=True)
    keys = [k for k in p if k.split(".")[0] in WM_PREFIXES]
    grads = torch.autograd.grad(out["model_loss"], [p[k] for k in keys])
    gn = 0.0
    for k, gr in zip(keys, grads):
        close(gr, g["grad/" + k], tol=2e-4, what="grad/" + k)
        gn += float((gr.double() ** 2).sum())
    assert abs(np.sqrt(gn) - float(g["model_grad_norm"])) <= 1e-4 * float(g["model_grad_norm"])


def behaviour(name, grad=False):
    g = load(name)
    cfg = common.path_config(name)
    p = tparams(name, grad)
    n = tnoise(name)
    start = {k: torch.from_numpy(g["post/" + k]) for k in ("stoch", "deter", "logit")}
    ema = torch.from_numpy(g["ema_vals_before"].copy())
    out = O.behavior_forward(cfg, p, start, n["act"], n["q_img"], ema)
    return g, cfg, p, out, ema


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_imagination_and_behaviour_forward(name):
    g, cfg, p, out, ema = behaviour(name)
    close(out["feats"], g["imag/feat"], what="feat")
    close(out["actions"], g["imag/action"], what="action")
    for k in ("stoch", "deter", "logit"):
        close(out["states"][k], g["imag/" + k], what="imag/" + k)
    close(out["reward"], g["imag/reward"], what="reward")
    close(out["actor_ent"], g["imag/actor_ent"], what="actor_ent")
    close(out["target"], g["imag/target"], what="target")
    close(out["weights"], g["imag/weights"], what="weights")
    close(out["value"], g["imag/value"], what="value")
    close(ema, g["ema_vals_after"], what="ema")
    close(out["actor_loss"], g["actor_loss"], tol=1e-5, what="actor_loss")
    close(out["value_loss"], g["value_loss"], tol=1e-5, what="value_loss")


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_behaviour_gradients(name):
    g, cfg, p, out, ema = behaviour(name, grad=True)
    akeys = [k for k in p if k.startswith("actor.")]
    vkeys = [k for k in p if k.startswith("value.")]
    ga = torch.autograd.grad(out["actor_loss"], [p[k] for k in akeys], retain_graph=True)
    gv = torch.autograd.grad(out["value_loss"], [p[k] for k in vkeys])
    for k, gr in zip(akeys, ga):
        close(gr, g["grad/" + k], tol=2e-4, what="grad/" + k)
    for k, gr in zip(vkeys, gv):
        close(gr, g["grad/" + k], tol=2e-4, what="grad/" + k)


@pytest.mark.parametrize("name", ["tiny", "tiny_onehot", "tiny_proprio", "tiny_both", "tiny_mixed"])
def test_full_update_matches_reference_train(name):
    """One oracle update (WM step, then behaviour on the UPDATED world model, as dreamer.py:194-200)
    reproduces the reference's own `_train` metrics and post-update parameters."""
    g = load(name)
    cfg = common.path_config(name)
    p = tparams(name, grad=True)
    n = tnoise(name)
    data = common.make_batch(name)
    out = O.wm_forward(cfg, p, data, n["q_prior"], n["q_post"])
    wkeys = [k for k in p if k.split(".")[0] in WM_PREFIXES]
    grads = torch.autograd.grad(out["model_loss"], [p[k] for k in wkeys])
    with torch.no_grad():
        st = dict(step=0, m=[torch.zeros_like(p[k]) for k in wkeys], v=[torch.zeros_like(p[k]) for k in wkeys])
        norm = O.clip_and_adam([p[k] for k in wkeys], list(grads), st, lr=1e-4, eps=1e-8, clip=1000.0)
    close(norm, g["train/model_grad_norm"], tol=1e-4, what="model_grad_norm")
    close(out["model_loss"], g["train/model_loss"], tol=1e-6, what="model_loss")
    for k in wkeys:
        close(p[k], g["after/" + k], tol=1e-6, what="after/" + k)
    # behaviour on the updated world model; slow critic EMA first (models.py:683-689)
    with torch.no_grad():
        for k in list(p):
            if k.startswith("value."):
                sk = "_slow_value." + k[len("value."):]
                p[sk].copy_(cfg.slow_target_fraction * p[k] + (1 - cfg.slow_target_fraction) * p[sk])
    start = {k: v.detach() for k, v in out["post"].items()}
    ema = torch.from_numpy(g["ema_vals_before"].copy())
    bout = O.behavior_forward(cfg, p, start, n["act"], n["q_img"], ema)
    close(bout["actor_loss"], g["train/actor_loss"], tol=1e-5, what="train/actor_loss")
    close(bout["value_loss"], g["train/value_loss"], tol=1e-5, what="train/value_loss")
    close(ema[0], g["train/EMA_005"], what="EMA_005")
    close(ema[1], g["train/EMA_095"], what="EMA_095")
    akeys = [k for k in p if k.startswith("actor.")]
    vkeys = [k for k in p if k.startswith("value.")]
    ga = torch.autograd.grad(bout["actor_loss"], [p[k] for k in akeys], retain_graph=True)
    gv = torch.autograd.grad(bout["value_loss"], [p[k] for k in vkeys])
    with torch.no_grad():
        for keys, gr, nm in ((akeys, ga, "actor"), (vkeys, gv, "value")):
            st = dict(step=0, m=[torch.zeros_like(p[k]) for k in keys], v=[torch.zeros_like(p[k]) for k in keys])
            norm = O.clip_and_adam([p[k] for k in keys], list(gr), st, lr=3e-5, eps=1e-5, clip=100.0)
            close(norm, g[f"train/{nm}_grad_norm"], tol=2e-4, what=nm + "_grad_norm")
    for k in akeys + vkeys + [k for k in p if k.startswith("_slow_value.")]:
        close(p[k], g["after/" + k], tol=1e-6, what="after/" + k)


@pytest.mark.parametrize("name", ["cfg2", "cfg1", "cfg3", "cfg4_b4", "cfg5_b4"])
def test_full_size_slices_and_checksums(name):
    """Full-size configs: stored row slices + whole-tensor checksums of the reference's outputs, world model and
    behaviour (imagination rows, lambda-returns, losses) -- this is what pins the oracle the GPU tests use at
    BASELINE sizes (cfg 3: deter 1024, 18-way one-hot actor, reinforce, batch 32)."""
    from tests import helpers as Hh

    g = load(name)
    torch.set_num_threads(Hh.host_threads())
    with torch.no_grad():
        cfg, p, n, data, out = wm_out(name)
    sel = slice(0, 2)
    close(out["embed"][sel], g["embed"], tol=1e-4, what="embed")
    # free-running 64-step sampled rollout on identical noise: the oracle's draws must be the reference's (same
    # host, same torch ops); a host on which an ulp flips a draw reports it here
    assert np.array_equal(out["post"]["stoch"][sel].numpy(), g["post/stoch"]), "oracle draws differ from the reference"
    for k in ("deter", "logit"):
        close(out["post"][k][sel], g["post/" + k], tol=1e-4, what="post/" + k)
        close(out["prior"][k][sel], g["prior/" + k], tol=1e-4, what="prior/" + k)
    close(out["model_loss"], g["model_loss"], tol=1e-5, what="model_loss")
    check_sum(g, "post/logit", out["post"]["logit"].numpy())
    for k, v in out["losses"].items():
        close(v, g["loss/" + k], tol=1e-4, what="loss/" + k)
    if cfg.encoder == "cnn":
        check_sum(g, "recon", out["recon"].numpy())
    # behaviour on the (not yet updated) world model: the golden file's imag/* pieces
    start = {k: v.detach() for k, v in out["post"].items()}
    ema = torch.zeros(2)
    with torch.no_grad():
        b = O.behavior_forward(cfg, p, start, n["act"], n["q_img"], ema)
    r8 = (slice(None), slice(0, 8))
    assert np.array_equal(b["states"]["stoch"][r8].numpy(), g["imag/stoch"]), "imagined draws differ from the reference"
    close(b["states"]["deter"][r8], g["imag/deter"], tol=1e-4, what="imag/deter")
    close(b["actions"][r8], g["imag/action"], tol=1e-4, what="imag/action")
    close(b["reward"][r8], g["imag/reward"], tol=1e-4, what="imag/reward")
    close(b["value"][r8], g["imag/value"], tol=1e-4, what="imag/value")
    close(b["target"][r8], g["imag/target"], tol=1e-4, what="imag/target")
    close(b["weights"][r8], g["imag/weights"], tol=1e-4, what="imag/weights")
    close(b["actor_ent"][r8], g["imag/actor_ent"], tol=1e-4, what="imag/actor_ent")
    check_sum(g, "imag/target", b["target"].numpy())
    check_sum(g, "imag/deter", b["states"]["deter"].numpy())
    close(b["actor_loss"], g["actor_loss"], tol=1e-5, what="actor_loss")
    close(b["value_loss"], g["value_loss"], tol=1e-5, what="value_loss")
    # (the file's ema_vals_after belongs to the full _train update that make_golden.py runs afterwards: the stored
    # array aliases the module buffer; it is compared in the full-update tests)


@pytest.mark.parametrize("name", ["cfg4_b4", "cfg5_b4"])
def test_crafter_width_gradients_and_update(name):
    """Crafter-size layers (configs.yaml:158-174: cnn_depth 96, deter 4096 / 2048, hidden = units = 1024; cfg5_b4
    also the 5-layer actor / reward / cont heads, one-hot actor, reinforce) at batch 4 x 8, horizon 5: every gradient
    of the three losses (whole-tensor checksums of the reference's), the three grad norms, and the reference's own
    `_train` metrics after its optimizer steps -- the pin of the oracle at BASELINE cfg 4 / cfg 5 widths."""
    from tests import helpers as Hh

    g = load(name)
    torch.set_num_threads(Hh.host_threads())
    r = Hh.oracle_update(name, piecewise=True)
    for k, v in r["wm_grads"].items():
        check_sum(g, "grad/" + k, v.numpy(), tol=2e-4)
    for k, v in r["actor_grads0"].items():
        check_sum(g, "grad/actor." + k[len("actor."):], v.numpy(), tol=2e-4)
    for k, v in r["value_grads0"].items():
        check_sum(g, "grad/value." + k[len("value."):], v.numpy(), tol=2e-4)
    close(r["model_grad_norm"], g["model_grad_norm"], tol=2e-3, what="model_grad_norm")
    close(r["wm"]["model_loss"], g["train/model_loss"], tol=1e-5, what="train/model_loss")
    close(r["beh"]["actor_loss"], g["train/actor_loss"], tol=2e-4, what="train/actor_loss")
    close(r["beh"]["value_loss"], g["train/value_loss"], tol=2e-4, what="train/value_loss")
    close(r["actor_grad_norm"], g["train/actor_grad_norm"], tol=2e-3, what="train/actor_grad_norm")
    close(r["value_grad_norm"], g["train/value_grad_norm"], tol=2e-3, what="train/value_grad_norm")
    close(r["ema"][0], g["train/EMA_005"], tol=2e-4, what="EMA_005")
    close(r["ema"][1], g["train/EMA_095"], tol=2e-4, what="EMA_095")


@pytest.mark.parametrize("name", ["tiny", "cfg2"])
def test_video_pred_matches_reference(name):
    """Open-loop prediction video (models.py:192-213) against the reference's own output."""
    g = load(name + "_video")
    cfg = common.path_config(name)
    p = tparams(name)
    n = {k: torch.from_numpy(v) for k, v in common.make_video_noise(name).items()}
    with torch.no_grad():
        v = O.video_pred(cfg, p, common.make_batch(name), n["q_prior"], n["q_post"], n["q_open"])
    assert tuple(v.shape) == tuple(g["meta/shape"])
    check_sum(g, "video", _np(v), tol=2e-5)
    if "video" in g.files:
        close(v, g["video"], what="video")
    else:
        T = v.shape[1]
        close(v[0, [0, 4, 5, T - 1]], g["video_rows"], what="video rows")


@pytest.mark.parametrize("name", ["tiny_p2e", "tiny_p2e_ac"])
def test_plan2explore_update_matches_reference(name):
    """The oracle's restatement of exploration.Plan2Explore.train (ensemble regression + Adam, intrinsic reward, the
    exploration behaviour's actor / critic update) against the reference's own run (tests/golden/make_golden.py run_p2e)."""
    from tests import helpers as Hh

    g = load(name)
    r = Hh.oracle_p2e_update(name)
    s = common.SHAPES[name]
    B, T = s["B"], s["T"]
    close(r["post"]["stoch"], g["post/stoch"], what="post/stoch")
    close(r["explorer_loss"], g["train/explorer_loss"], tol=1e-6, what="explorer_loss")
    close(r["explorer_grad_norm"], g["train/explorer_grad_norm"], tol=1e-4, what="explorer_grad_norm")
    for k, v in r["explorer_grads"].items():
        close(v, g["grad/" + k], tol=2e-4, what="grad/" + k)
    b = r["beh"]
    close(b["reward"], g["imag/reward"], tol=2e-5, what="imag/reward")
    close(b["actions"], g["imag/action"], tol=2e-5, what="imag/action")
    close(b["actor_loss"], g["train/actor_loss"], tol=1e-5, what="actor_loss")
    close(b["value_loss"], g["train/value_loss"], tol=1e-5, what="value_loss")
    close(r["ema"][0], g["train/EMA_005"], what="EMA_005")
    close(r["ema"][1], g["train/EMA_095"], what="EMA_095")
    close(r["actor_grad_norm"], g["train/actor_grad_norm"], tol=2e-4, what="actor_grad_norm")
    close(r["value_grad_norm"], g["train/value_grad_norm"], tol=2e-4, what="value_grad_norm")
    for nm in ("actor", "value"):
        for k, v in r[nm + "_grads"].items():
            close(v, g["grad/_behavior." + k], tol=2e-4, what="grad/_behavior." + k)
    for k, v in r["p2e_after"].items():
        close(v, g["after/" + k], tol=1e-6, what="after/" + k)
