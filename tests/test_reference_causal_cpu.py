"""The reference's own causal world models -- scm_world_model.WorldModelWithSCM (scm_world_model.py:407) and
causal_VAE.CausalVAE_WorldModel (causal_VAE.py:858) -- build on this repo's `networks` / `tools`.
They stay the integrator's files; what is pinned here is that the class surface they build on (RSSM / MultiEncoder /
MultiDecoder / MLP constructors and private members, tools.Optimizer) is the reference's.  Every constructor call
they make at the tiny config was recorded from the reference itself (tests/golden/causal_construct.json, written by
tests/golden/make_causal_golden.py from a reference checkout) and is replayed here on these modules."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "causal_construct.json")))
SURFACE = json.load(open(os.path.join(HERE, "golden", "surface.json")))
CAUSAL_FILES = ("scm_world_model.py", "causal_VAE.py")
# SCMRSSM's own methods (tests/test_surface_cpu.py OUTSIDE): not members of networks.RSSM
SCM_ONLY = {"intervene", "remove_intervention"}


def decode(v, params):
    if isinstance(v, dict):
        if set(v) == {"tuple"}:
            return tuple(decode(x, params) for x in v["tuple"])
        if set(v) == {"params"}:
            return params()
        if set(v) == {"device"}:
            import torch

            return torch.device(v["device"])
        return {k: decode(x, params) for k, x in v.items()}
    if isinstance(v, list):
        return [decode(x, params) for x in v]
    return v


def test_reference_causal_world_models_construct_on_these_modules():
    import torch

    import networks
    import tools

    mods = {"networks": networks, "tools": tools}
    rssm_used = {a for a, sites in SURFACE["RSSM"].items() if any(s.startswith(CAUSAL_FILES) for s in sites)}
    assert set(FIXTURE) == {"WorldModelWithSCM", "CausalVAE_WorldModel"}
    for model, rec in FIXTURE.items():
        calls = rec["calls"]
        assert {c["cls"] for c in calls} == {"networks.RSSM", "networks.MultiEncoder", "networks.MultiDecoder",
                                             "networks.MLP", "tools.Optimizer"}, model
        built = []

        def params():
            return (p for m in built for p in m.parameters())

        for c in calls:
            where = f"{model}.{c['path']}"
            mname, cname = c["cls"].split(".")
            cls = getattr(mods[mname], cname)
            obj = cls(*decode(c["args"], params), **decode(c["kwargs"], params))
            assert isinstance(obj, cls), where
            if isinstance(obj, torch.nn.Module):
                assert sum(p.numel() for p in obj.parameters()) == c["numel"], f"{where}: parameter count"
                for sub, tname in c["children"].items():
                    got = obj.get_submodule(sub)
                    assert isinstance(got, getattr(networks, tname.split(".")[1])), f"{where}.{sub} is {type(got)}"
                built.append(obj)
            if isinstance(obj, networks.RSSM):
                assert isinstance(obj._cell, networks.GRUCell), where
                for a in sorted(rssm_used - SCM_ONLY):
                    assert hasattr(obj, a), f"{where}: RSSM.{a} (used by the causal models) is missing"
        assert isinstance(obj, tools.Optimizer) and calls[-1]["path"] == "_model_opt", model
        assert sum(p.numel() for m in built for p in m.parameters()) > 0, model
