"""The Plan2Explore fixtures of the continuous-latent configurations (tests/golden/tiny_gauss_p2e*.npz, written by
tests/golden/make_golden_gauss_p2e.py from the reference): they load without pickle, hold exactly the arrays
gauss_p2e_common.fixture_layout declares, with the shapes of the two configurations, and stay within the size limit
for committed files.  No GPU, no reference."""
import os

import numpy as np
import pytest

from tests.golden import common, gauss_common as GC, gauss_p2e_common as GP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_BYTES = 1 << 20  # no committed file above 1 MiB


@pytest.fixture(scope="module", params=GP.NAMES)
def fixture(request):
    path = os.path.join(GOLDEN, request.param + ".npz")
    return request.param, path, np.load(path, allow_pickle=False)


def test_configurations_are_tiny_gauss_with_the_p2e_settings():
    base = common.SHAPES[GP.BASE]
    assert base["discrete"] == 0
    for name in GP.NAMES:
        s = common.SHAPES[name]
        assert {k: v for k, v in s.items() if k != "p2e"} == base
        assert s["p2e"] == GP.P2E[name]
    a, b = (GP.P2E[n] for n in GP.NAMES)
    assert (a["disag_target"], a["disag_action_cond"], a["expl_extr_scale"]) == ("stoch", False, 0.0)
    assert (b["disag_target"], b["disag_action_cond"]) == ("feat", True) and b["expl_extr_scale"] != 0
    # the settings of the categorical fixtures, but for the target that only continuous latents make well-formed
    assert a == common.SHAPES["tiny_p2e"]["p2e"]
    assert dict(b, disag_target="deter") == common.SHAPES["tiny_p2e_ac"]["p2e"]


def test_fixture_holds_the_declared_arrays(fixture):
    name, path, g = fixture
    lay = GP.fixture_layout(name)
    assert set(g.files) == set(lay), set(g.files) ^ set(lay)
    assert str(g["meta/name"]) == name
    for k, shp in lay.items():
        if k == "meta/name":
            continue
        assert tuple(g[k].shape) == shp, (k, g[k].shape, shp)
        assert g[k].dtype == (np.float64 if k.startswith("train/") else np.float32), (k, g[k].dtype)
        assert np.all(np.isfinite(g[k])), k
    assert os.path.getsize(path) <= MAX_BYTES


def test_fixture_shapes_follow_the_configuration(fixture):
    name, _, g = fixture
    s = common.SHAPES[name]
    c = s["p2e"]
    S, De, A = s["stoch"], s["deter"], s["A"]
    width = {"stoch": S, "feat": S + De}[c["disag_target"]]
    inp = S + De + (A if c["disag_action_cond"] else 0)
    members = {k.split(".")[1] for k in g.files if k.startswith("grad/_networks.")}
    assert members == {str(i) for i in range(c["disag_models"])}
    for i in range(c["disag_models"]):
        assert g[f"grad/_networks.{i}.layers.NoName_linear0.weight"].shape == (c["disag_units"], inp)
        assert g[f"after/_networks.{i}.mean_layer.weight"].shape == (width, c["disag_units"])
        assert f"grad/_networks.{i}.layers.NoName_linear{c['disag_layers'] - 1}.weight" in g.files
        assert f"grad/_networks.{i}.layers.NoName_linear{c['disag_layers']}.weight" not in g.files
    assert g["imag/feat"].shape[-1] == S + De and g["post/stoch"].shape == (s["B"], s["T"], S)
    # the update moved every trained parameter away from the deterministic start, and left nothing else behind
    pw = GP.make_p2e_weights(name)
    for k, w in pw.items():
        moved = not np.array_equal(g["after/" + k], w)
        assert moved, k
    # the imagined start states are the stored posterior (rows b * T + t)
    np.testing.assert_array_equal(g["imag/feat"][0], np.concatenate([g["post/stoch"], g["post/deter"]], -1).reshape(-1, S + De))
    # the recorded noise is regenerated, not stored: gauss_common's tapes at these shapes
    nz = GC.make_noise(name, seed=GP.NOISE_SEED_X)
    assert nz["act"].shape == g["imag/action"].shape and nz["q_img"].shape == (s["H"], s["B"] * s["T"], S)
