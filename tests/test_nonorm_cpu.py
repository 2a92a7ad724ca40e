"""CPU-side checks of norm / encoder.norm / decoder.norm: False: the parameter tables of the fixtures, the public classes'
module structure and state_dict surface against the reference's (tests/golden/nonorm_surface.json, written by
tests/golden/make_golden_nonorm.py), and what the parameter containers hand to the engines.  No kernel launches."""
import json
import os

import numpy as np
import pytest
import torch

from tests import nonorm_helpers as N
from tests.golden import common
from tests.golden import nonorm_common as NC

GOLDEN = N.GOLDEN


def _surface(wm, beh):
    sd = {**dict(wm.state_dict()), **{k: v for k, v in beh.state_dict().items()
                                       if not k.startswith("_world_model.") and k != "ema_vals"}}
    return {k: list(v.shape) for k, v in sd.items()}


def _build(row, norm, enc_norm, dec_norm):
    import models
    from dv3hip import shapes

    cfg = shapes.make_config(row, "cpu")
    cfg.norm, cfg.encoder["norm"], cfg.decoder["norm"] = norm, enc_norm, dec_norm
    wm = models.WorldModel(shapes.obs_space(row), None, 0, cfg)
    return cfg, wm, models.ImagBehavior(cfg, wm)


@pytest.mark.parametrize("combo,key", NC.surface_combos(), ids=[k for _, k in NC.surface_combos()])
def test_state_dict_surface_equals_the_reference(combo, key):
    """Names, shapes AND order of WorldModel + ImagBehavior's state_dict for every combination of the three keys."""
    ref = json.load(open(os.path.join(GOLDEN, "nonorm_surface.json")))[key]
    _, wm, beh = _build(NC.SURFACE_ROW, *combo)
    got = _surface(wm, beh)
    assert got == ref, sorted(set(got) ^ set(ref))
    assert sorted(got) == sorted(NC.shapes_of(common.SHAPES[NC.SURFACE_ROW], *combo))
    # LayerNorm modules exactly in the groups whose key is True
    ln = lambda m: any(isinstance(x, torch.nn.LayerNorm) for x in m.modules())
    n, e, d = combo
    assert ln(wm.encoder) == e and ln(wm.heads["decoder"]) == d
    for m in (wm.dynamics, wm.heads["reward"], wm.heads["cont"], beh.actor, beh.value, beh._slow_value):
        assert ln(m) == n


def test_no_bias_appears_and_the_sequentials_renumber():
    _, wm, beh = _build(NC.SURFACE_ROW, False, False, False)
    sd = _surface(wm, beh)
    assert "dynamics._img_in_layers.0.weight" in sd and not any(k.startswith("dynamics._img_in_layers.1") for k in sd)
    assert not any("norm" in k for k in sd)
    assert [k for k in sd if k.startswith("encoder._cnn.layers.")] == [f"encoder._cnn.layers.{i}.weight" for i in (0, 2, 4, 6)]
    dec = [k for k in sd if k.startswith("heads.decoder._cnn.layers.")]
    assert dec == [f"heads.decoder._cnn.layers.{i}.weight" for i in (0, 2, 4, 6)] + ["heads.decoder._cnn.layers.6.bias"]
    # the only biases are the ones norm: True has as well: the stat layers, the head Linears, the decoder's last layer
    with_norm = _surface(*_build(NC.SURFACE_ROW, True, True, True)[1:])
    lin_bias = lambda t: [k for k in t if k.endswith(".bias") and len(t[k[:-4] + "weight"]) >= 2]
    assert lin_bias(sd) == [k for k in sd if k.endswith(".bias")] and len(lin_bias(sd)) == len(lin_bias(with_norm))
    assert [type(m).__name__ for m in wm.dynamics._img_in_layers] == ["Linear", "SiLU"]
    assert [n for n, _ in wm.dynamics._cell.layers.named_children()] == ["GRU_linear"]


def test_parameter_containers_hand_none_for_a_missing_layernorm():
    _, wm, beh = _build(NC.SURFACE_ROW, False, True, False)
    P = wm.dynamics.params()
    for L in (P.img_in, P.gru, P.img_out, P.obs_out, *beh.actor.trunk_params(), *beh.value.trunk_params(),
              *wm.heads["reward"].trunk_params()):
        assert L.g is None and L.b is None
    assert all(L.g is not None for L in wm.encoder._cnn.conv_params())
    assert all(L.g is not None for L in wm.encoder._mlp.trunk_params())
    dec = wm.heads["decoder"]._cnn.conv_params()
    assert [L.g is None for L in dec] == [True] * 4 and [L.out for L in dec] == [False, False, False, True]
    assert all(L.g is None for L in wm.heads["decoder"]._mlp.trunk_params())
    # with the LayerNorm the output layer is still told apart by its bias
    dec = _build(NC.SURFACE_ROW, True, True, True)[1].heads["decoder"]._cnn.conv_params()
    assert [L.g is None for L in dec] == [False, False, False, True] and [L.out for L in dec] == [False, False, False, True]


def test_direct_construction_is_opt_in():
    """A bare norm=False keeps raising (the message names the default and the scope); inside networks.layernorm_free()
    the same calls build the reference's modules; the scope is re-entrant and gone on exit, also after an error."""
    import networks

    mk = dict(
        gru=lambda: networks.GRUCell(8, 8, norm=False),
        rssm=lambda: networks.RSSM(4, 16, 16, 1, 4, norm=False, num_actions=3, embed=8),
        mlp=lambda: networks.MLP(8, (3,), 2, 16, device="cpu", norm=False),
        enc=lambda: networks.ConvEncoder((64, 64, 3), 2, norm=False),
        dec=lambda: networks.ConvDecoder(20, (3, 64, 64), 2, norm=False))
    ln = lambda m: any(isinstance(x, torch.nn.LayerNorm) for x in m.modules())
    for nm, f in mk.items():
        with pytest.raises(NotImplementedError, match="norm=True.*layernorm_free"):
            f()
        with networks.layernorm_free():
            with networks.layernorm_free():
                assert not ln(f()), nm
            assert not ln(f()), nm
        with pytest.raises(NotImplementedError, match="layernorm_free"):
            f()
    with pytest.raises(ZeroDivisionError):
        with networks.layernorm_free():
            1 / 0
    with pytest.raises(NotImplementedError):
        mk["mlp"]()
    # norm=True is untouched by the scope
    with networks.layernorm_free():
        assert ln(networks.MLP(8, (3,), 2, 16, device="cpu")) and ln(networks.GRUCell(8, 8))


def test_models_open_the_scope_only_for_a_config_that_asks():
    import models
    import networks

    assert networks._LN_FREE[0] == 0
    _build(NC.SURFACE_ROW, False, True, True)
    assert networks._LN_FREE[0] == 0
    assert isinstance(models._norm_scope(N.Hh.make_config("tiny", "cpu")), type(__import__("contextlib").nullcontext()))
    assert isinstance(models._norm_scope(N.Hh.make_config("tiny_nonorm_mix", "cpu")), networks.layernorm_free)


def test_other_refusals_stay():
    import networks

    with pytest.raises(NotImplementedError, match="update_bias"):
        networks.GRUCell(8, 8, norm=False, update_bias=0)
    with pytest.raises(NotImplementedError, match="rec_depth"):
        networks.RSSM(4, 16, 16, 2, 4, norm=False, num_actions=3, embed=8)
    with pytest.raises(NotImplementedError, match="initial"):
        networks.RSSM(4, 16, 16, 1, 4, norm=False, initial="zeros", num_actions=3, embed=8)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        networks.ConvEncoder((64, 64, 3), 2, norm=False, kernel_size=3)
    with pytest.raises(NotImplementedError, match="cnn_sigmoid"):
        networks.ConvDecoder(20, (3, 64, 64), 2, norm=False, cnn_sigmoid=True)


@pytest.mark.parametrize("name", NC.NAMES)
def test_fixture_tables(name):
    s = common.SHAPES[name]
    assert set(NC.norm_keys(s)) <= {True, False} and not all(NC.norm_keys(s))
    g = N.gold(name)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)
    assert [bool(x) for x in g["meta/norm_keys"]] == list(NC.norm_keys(s))
    assert 0.0 < float(g["meta/gru_pre_absmax"]) <= NC.GRU_PRE_MAX
    missing = [k for k in N.fixture_keys(name) if k not in set(g.files)]
    assert not missing, missing[:10]
    w = NC.make_weights(name)
    for k, shp in NC.param_shapes(name).items():
        assert w[k].shape == tuple(shp) and w[k].dtype == np.float32
        assert g["after/" + k].shape == tuple(shp)
    cfg = N.Hh.make_config(name, "cpu")
    assert (cfg.norm, cfg.encoder["norm"], cfg.decoder["norm"]) == NC.norm_keys(s)


def test_benchmark_shape_is_cfg2_without_layernorm():
    from dv3hip import shapes

    a, b = dict(shapes.SHAPES["cfg2"]), dict(shapes.SHAPES["cfg2_nonorm"])
    assert NC.norm_keys(b) == (False, False, False)
    for k in ("norm", "enc_norm", "dec_norm"):
        b.pop(k)
    assert a == b
    cfg = shapes.make_config("cfg2_nonorm", "cpu")
    assert (cfg.norm, cfg.encoder["norm"], cfg.decoder["norm"]) == (False, False, False)
    assert shapes.make_config("cfg2", "cpu").norm is True


def test_plan2explore_takes_the_autograd_route_without_norm():
    import exploration
    import models
    from dv3hip import shapes

    cfg = shapes.make_config("tiny_p2e", "cpu")
    cfg.norm = False
    wm = models.WorldModel(shapes.obs_space("tiny_p2e"), None, 0, cfg)
    p2e = exploration.Plan2Explore(cfg, wm, lambda f, s, a: None)
    assert "norm" in p2e.fused_reason() and not p2e._wants_fused()
    # the ensemble is built as the reference builds it (exploration.py:66-73 passes no `norm`: its members keep theirs)
    assert any(isinstance(m, torch.nn.LayerNorm) for m in p2e._networks.modules())
    assert not any(isinstance(m, torch.nn.LayerNorm) for m in p2e.actor.modules())
