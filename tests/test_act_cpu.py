"""Layer activations other than SiLU, the parts that need no GPU: the four shapes build a config, ops.ACT_CODES is the
header's table, unknown activations and norm: False raise, and every new fixture holds what the path test reads."""
import os
import re

import numpy as np
import pytest

from tests import act_helpers as A
from tests import helpers as Hh
from tests.golden import act_common as AC
from tests.golden import common

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", AC.NAMES)
def test_shapes_build_a_config(name):
    s = common.SHAPES[name]
    cfg = Hh.make_config(name, device="cpu")
    assert (cfg.act, cfg.encoder["act"], cfg.decoder["act"]) == (s["act"], s["enc_act"], s["dec_act"])
    assert cfg.dyn_discrete == s["discrete"] and cfg.imag_gradient == s["imag_gradient"]
    assert cfg.norm is True and cfg.encoder["norm"] is True and cfg.decoder["norm"] is True
    assert (getattr(cfg, "expl_behavior", "greedy") == "plan2explore") == ("p2e" in s)
    # the default stays today's
    base = Hh.make_config("tiny", device="cpu")
    assert (base.act, base.encoder["act"], base.decoder["act"]) == ("SiLU", "SiLU", "SiLU")


def test_the_shapes_are_what_the_issue_lists():
    S = common.SHAPES
    assert {k: S["tiny_elu"][k] for k in ("act", "enc_act", "dec_act", "actor_dist", "imag_gradient")} == dict(
        act="ELU", enc_act="ELU", dec_act="ELU", actor_dist="normal", imag_gradient="dynamics")
    assert {k: S["tiny_elu"][k] for k in ("stoch", "discrete", "deter", "hidden", "units", "B", "T", "H")} == \
        {k: S["tiny"][k] for k in ("stoch", "discrete", "deter", "hidden", "units", "B", "T", "H")}
    m = S["tiny_actmix"]
    assert (m["act"], m["enc_act"], m["dec_act"], m["actor_dist"], m["imag_gradient"], m["encoder"]) == \
        ("GELU", "Mish", "ReLU", "onehot", "reinforce", "both")
    assert S["tiny_gauss_tanh"]["discrete"] == 0 and S["tiny_gauss_tanh"]["act"] == "Tanh"
    assert S["tiny_p2e_elu"]["p2e"] == S["tiny_p2e"]["p2e"] and S["tiny_p2e_elu"]["act"] == "ELU"


def test_act_codes_match_the_header():
    from dv3hip import ops

    text = open(os.path.join(REPO, "include", "dv3hip.h")).read()
    rows = re.findall(r"^ \*\s+(\d)\s+(none|SiLU|ReLU|ELU|GELU|Tanh|Mish)\s", text, flags=re.M)
    assert {n: int(c) for c, n in rows} == ops.ACT_CODES and len(rows) == 7
    defs = dict(re.findall(r"^#define DV3_ACT_(\w+) (\d)$", text, flags=re.M))
    assert {k.upper(): v for k, v in ops.ACT_CODES.items()} == {k: int(v) for k, v in defs.items()}
    common_h = open(os.path.join(REPO, "dreamerv3-torch_amd", "csrc", "dv3_common.h")).read()
    assert dict(re.findall(r"^#define DV3_ACT_(\w+) (\d)$", common_h, flags=re.M)) == defs
    assert ops.act_code(True) == 1 and ops.act_code(False) == 0 and ops.act_code("Mish") == 6 and ops.act_code(4) == 4
    import torch

    assert ops.act_code(torch.nn.ELU) == 3 and ops.act_code(torch.nn.Tanh()) == 5


def test_unknown_activation_and_norm_false_raise():
    import networks
    from dv3hip import ops

    with pytest.raises(NotImplementedError, match="Softsign.*SiLU.*ReLU.*ELU.*GELU.*Tanh.*Mish"):
        ops.act_code("Softsign")
    mk = dict(
        rssm=lambda **kw: networks.RSSM(4, 16, 16, 1, 4, num_actions=3, embed=8, **kw),
        mlp=lambda **kw: networks.MLP(8, (3,), 2, 16, device="cpu", **kw),
        enc=lambda **kw: networks.ConvEncoder((64, 64, 3), 2, **kw),
        dec=lambda **kw: networks.ConvDecoder(20, (3, 64, 64), 2, **kw))
    for nm, f in mk.items():
        with pytest.raises(NotImplementedError, match="Softsign"):
            f(act="Softsign")
        with pytest.raises(NotImplementedError, match="norm=True"):
            f(norm=False)
        mod = f(act="GELU")
        kinds = {type(x).__name__ for x in mod.modules()} & {"SiLU", "ReLU", "ELU", "GELU", "Tanh", "Mish"}
        assert kinds == {"GELU"}, (nm, kinds)
    # child order and state_dict keys are the reference's, whatever the activation
    a, b = mk["mlp"](act="ELU"), mk["mlp"]()
    assert list(a.state_dict()) == list(b.state_dict()) and [n for n, _ in a.layers.named_children()] == \
        [n for n, _ in b.layers.named_children()]
    r = mk["rssm"](act="Tanh")
    assert [type(m).__name__ for m in r._img_in_layers] == ["Linear", "LayerNorm", "Tanh"]
    assert r.params().img_in.act == r.params().obs_out.act == r.params().img_out.act == 5 and r.params().gru.act == 1


@pytest.mark.parametrize("name", AC.NAMES)
def test_fixture_holds_the_keys_the_path_test_reads(name):
    path = os.path.join(A.GOLDEN, name + ".npz")
    assert os.path.getsize(path) < (1 << 20)
    g = np.load(path, allow_pickle=False)
    have = set(g.files)
    missing = [k for k in A.fixture_keys(name) if k not in have]
    assert not missing, missing[:10]
    assert bool(g["meta/full"]) and str(g["meta/name"]) == name
    assert int(g["meta/weight_seed"]) == AC.WEIGHT_SEED.get(name, 0)
    s = common.SHAPES[name]
    assert g["post/stoch"].shape[:2] == (s["B"], s["T"]) and np.isfinite(g["model_loss"])
    if "ReLU" in (s["act"], s["enc_act"], s["dec_act"]):
        assert float(g["meta/relu_min"]) > AC.RELU_MARGIN
    if name == "tiny_elu":
        v = np.load(os.path.join(A.GOLDEN, name + "_video.npz"), allow_pickle=False)
        assert {"sum/video", "meta/shape", "video_model"} <= set(v.files)
