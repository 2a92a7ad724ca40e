"""CPU-side checks of the continuous-latent (dyn_discrete: 0) feature: the fixtures written from the reference load
and hold what the GPU tests read, networks.RSSM(discrete=0) constructs with the reference's parameter names and shapes,
the shape table round-trips through make_config, and the library exports the Gaussian kernels."""
import os

import numpy as np
import pytest
import torch

from tests.golden import common, gauss_common as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["tiny_gauss", "tiny_gauss_onehot", "cfg2_gauss"]


def _gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_loads_and_holds_the_keys(name):
    g = _gold(name)
    files = set(g.files)
    s = common.SHAPES[name]
    full = bool(g["meta/full"])
    assert full == name.startswith("tiny")
    for grp in ("post/", "prior/", "imag/"):
        for k in ("stoch", "deter", "mean", "std"):
            if grp + k == "prior/deter" and not full:
                continue  # (prior deter IS post deter: stored once at full size)
            assert grp + k in files and "sum/" + grp + k in files, grp + k
        assert grp + "logit" not in files
    for k in ("embed", "recon", "reward_logits", "cont_logit", "loss/image", "loss/reward", "loss/cont", "kl_value",
              "kl_loss", "dyn_loss", "rep_loss", "prior_ent", "post_ent", "model_loss", "model_grad_norm", "imag/feat",
              "imag/action", "imag/reward", "imag/target", "imag/weights", "imag/value", "imag/actor_ent", "actor_loss",
              "value_loss"):
        assert k in files, k
    shapes = GC.param_shapes(name)
    for k in shapes:
        head = k.split(".")[0]
        if head in ("encoder", "dynamics", "heads"):
            assert "sum/grad/" + k in files, k
        elif head in ("actor", "value"):
            assert "sum/grad/" + k in files, k
        assert "sum/after/" + k in files and "sum/after2/" + k in files, k
        if full:
            assert tuple(g["w/" + k].shape) == shapes[k] and tuple(g["after2/" + k].shape) == shapes[k], k
    if not full:  # sampled elements and delta checksums of every gradient / Adam-updated parameter
        for grp in ("grad", "after", "after2"):
            lay = GC.sample_layout(name, grp)
            assert g["smp/" + grp].size == sum(idx.size for _, idx in lay.values())
            assert all(idx.size == min(GC.SAMPLE, int(np.prod(shapes[k])) if k in shapes else 2) for k, (_, idx) in lay.items())
        w0 = GC.make_weights(name)
        off, idx = GC.sample_layout(name, "after")["dynamics.W"]
        step = g["smp/after"][off:off + idx.size] - w0["dynamics.W"].reshape(-1)[idx]
        assert 0 < np.abs(step).max() <= 1.01e-4  # an lr-sized Adam step is visible in the stored elements
        for grp in ("after", "after2"):
            d = g["sum/delta/" + grp]
            assert d.shape == (len(GC.delta_names(name)), 3) and (d[:, 1] > 0).all()
    for tr in ("train/", "train2/"):
        for k in ("model_loss", "model_grad_norm", "kl", "prior_ent", "post_ent", "dyn_loss", "rep_loss", "actor_loss",
                  "value_loss", "actor_grad_norm", "value_grad_norm"):
            assert tr + k in files, tr + k
    for tag in ("train", "eval"):
        for t in range(GC.POLICY_STEPS):
            for k in ("action", "logprob", "stoch", "deter", "mean", "std"):
                assert f"policy/{tag}/{t}/{k}" in files
            assert g[f"policy/{tag}/{t}/stoch"].shape == (GC.POLICY_ENVS, s["stoch"])
        assert np.array_equal(g[f"policy/eval/{t}/stoch"], g[f"policy/eval/{t}/mean"])
    # free-bits coverage: per-step KL values on both sides of kl_free = 1
    kl = g["kl_value"]
    assert kl.shape == (s["B"], s["T"]) and (kl < 1.0).any() and (kl > 1.0).any()
    assert np.array_equal(g["dyn_loss"], np.maximum(kl, 1.0))
    if full:
        w = GC.make_weights(name)
        for k, v in w.items():
            assert np.array_equal(g["w/" + k], v), k
        n = GC.make_noise(name)
        for k, v in n.items():
            assert np.array_equal(g["noise/" + k], v), k
        assert np.array_equal(g["sum/data/image"], common.checksum(GC.make_batch(name)["image"]))
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 1 << 20


def test_video_fixture_loads():
    g = np.load(os.path.join(GOLDEN, "tiny_gauss_video.npz"), allow_pickle=False)
    s = common.SHAPES["tiny_gauss"]
    assert tuple(g["meta/shape"]) == (s["B"], s["T"], 192, 64, 3)
    assert g["video_model"].shape == (s["B"], s["T"], 64, 64, 3)


@pytest.mark.parametrize("name", NAMES)
def test_rssm_constructs_with_the_references_parameters(name):
    """networks.RSSM(discrete=0) on the CPU: state_dict names and shapes are the reference's (the fixture's w/ keys)."""
    import networks

    s = common.SHAPES[name]
    E = s["cnn_depth"] * 8 * 16
    rssm = networks.RSSM(stoch=s["stoch"], deter=s["deter"], hidden=s["hidden"], discrete=0,
                         mean_act=s.get("mean_act", "none"), std_act=s.get("std_act", "sigmoid2"), min_std=0.1,
                         num_actions=s["A"], embed=E, device="cpu")
    want = {k[len("dynamics."):]: v for k, v in GC.param_shapes(name).items() if k.startswith("dynamics.")}
    got = {k: tuple(v.shape) for k, v in rssm.state_dict().items()}
    assert got == want
    g = _gold(name)
    if bool(g["meta/full"]):
        assert got == {k[len("w/dynamics."):]: tuple(g[k].shape) for k in g.files if k.startswith("w/dynamics.")}
    assert got["_img_in_layers.0.weight"] == (s["hidden"], s["stoch"] + s["A"])
    assert got["_imgs_stat_layer.weight"] == got["_obs_stat_layer.weight"] == (2 * s["stoch"], s["hidden"])
    with pytest.raises(NotImplementedError):
        networks.RSSM(stoch=8, deter=16, hidden=16, discrete=0, std_act="exp", num_actions=3, embed=E, device="cpu")


@pytest.mark.parametrize("name", NAMES)
def test_make_config_round_trips_and_the_models_construct(name):
    import models
    from dv3hip import shapes

    s = shapes.SHAPES[name]
    cfg = shapes.make_config(name, "cpu")
    assert cfg.dyn_discrete == 0 and cfg.dyn_stoch == s["stoch"] and cfg.dyn_deter == s["deter"]
    assert cfg.dyn_mean_act == s.get("mean_act", "none") and cfg.dyn_std_act == s.get("std_act", "sigmoid2")
    assert cfg.dyn_min_std == 0.1 and cfg.batch_size == s["B"] and cfg.batch_length == s["T"]
    assert (cfg.actor["dist"] == "onehot") == (s["actor_dist"] == "onehot")
    wm = models.WorldModel(shapes.obs_space(name), None, 0, cfg)
    beh = models.ImagBehavior(cfg, wm)
    sd = {k: tuple(v.shape) for k, v in wm.state_dict().items()}
    sd.update({k: tuple(v.shape) for k, v in beh.state_dict().items()
               if not k.startswith("_world_model.") and k != "ema_vals"})
    assert sd == GC.param_shapes(name)
    batch = shapes.synthetic_batch(name)
    assert batch["image"].shape == (s["B"], s["T"], 64, 64, 3) and batch["action"].shape == (s["B"], s["T"], s["A"])


def test_the_library_exports_the_gaussian_kernels():
    from dv3hip import _lib

    decls = _lib.parse_header()
    lib = _lib.load()
    for fn in ("dv3_gauss_head_fwd", "dv3_gauss_head_bwd", "dv3_gauss_kl_fwd", "dv3_gauss_kl_bwd"):
        assert fn in decls and hasattr(lib, fn)
    # rejected before any launch (safe without a GPU)
    assert lib.dv3_gauss_head_fwd(None, None, None, 0, None, None, None, None, 4, 8, 0, 0, 0.1, 0, None, None, None,
                                  None) == 10001
    assert lib.dv3_gauss_head_bwd(None, None, None, None, None, None, 4, 8, 0, 0, 0, 0, None) == 10001
    assert lib.dv3_gauss_kl_fwd(None, None, None, None, None, None, None, 4, 8, None) == 10001
    assert lib.dv3_gauss_kl_bwd(None, None, None, None, None, None, None, None, None, 4, 8, 1.0, 0.5, 0.1, 1.0, 0, 0,
                                None) == 10001


def test_noise_tapes_follow_the_references_draw_order():
    n = GC.make_noise("tiny_gauss")
    s = common.SHAPES["tiny_gauss"]
    tape = GC.observe_tape(n)
    assert len(tape) == 2 * s["T"] and tape[0].shape == (s["B"], s["stoch"]) and tape[1] is not None
    assert np.array_equal(tape[0], n["q_prior"][0]) and np.array_equal(tape[1], n["q_post"][0])
    tape = GC.imagine_tape(n)
    assert tape[0].shape == (s["B"] * s["T"], s["A"]) and tape[1].shape == (s["B"] * s["T"], s["stoch"])


def test_latent_distribution_object_is_not_the_actors():
    import tools

    d = tools.NormalLatent(torch.zeros(2, 3), torch.ones(2, 3))
    assert d.mode() is d.mean and d.stddev.shape == (2, 3)
    assert tools.ContDist.__init__.__code__.co_varnames[:5] == ("self", "mean_raw", "std_raw", "min_std", "max_std")
