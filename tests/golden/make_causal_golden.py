#!/usr/bin/env python3
"""Causal-model fixture: every call the reference's causal world models --
scm_world_model.WorldModelWithSCM (scm_world_model.py:407) and causal_VAE.CausalVAE_WorldModel (causal_VAE.py:858) --
make to a `networks` / `tools` constructor of THIS repo while they are built at the tiny config: class, arguments,
where the piece lands in the model, the `networks` classes inside it and its parameter count.  Needs a reference
checkout (the argument): imports its files from where they lie, behind the package on sys.path (networks / tools /
models resolve to the MI355X modules); nothing of the reference is copied.  Writes tests/golden/causal_construct.json, which
tests/test_reference_causal_cpu.py replays.

    python tests/golden/make_causal_golden.py REFERENCE_CHECKOUT
"""
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else sys.exit(__doc__)
sys.path.insert(0, os.path.join(REPO, "dreamerv3-torch_amd"))
sys.path.insert(0, REPO)
sys.path.append(REF)  # behind the package

import torch  # noqa: E402

import networks  # noqa: E402
import tools  # noqa: E402
from dv3hip import shapes  # noqa: E402

CLASSES = {"networks.RSSM": networks.RSSM, "networks.MultiEncoder": networks.MultiEncoder,
           "networks.MultiDecoder": networks.MultiDecoder, "networks.MLP": networks.MLP,
           "tools.Optimizer": tools.Optimizer}
PARAMS = {"params": "parameters of the model under construction"}


def encode(v):
    if isinstance(v, tuple):
        return {"tuple": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    if isinstance(v, dict):
        return {str(k): encode(x) for k, x in v.items()}
    if isinstance(v, torch.device):
        return {"device": str(v)}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if hasattr(v, "__next__"):  # self.parameters() of tools.Optimizer
        return PARAMS
    raise TypeError(f"cannot record {type(v)}")


def networks_children(obj):
    return {n: f"networks.{type(m).__name__}" for n, m in obj.named_modules()
            if n and type(m).__module__ == "networks"}


def main():
    calls = []
    originals = {}
    for name, cls in CLASSES.items():
        originals[name] = cls.__init__

        def rec(self, *args, _name=name, _init=cls.__init__, **kwargs):
            entry = {"cls": _name, "args": encode(args), "kwargs": encode(kwargs)}
            calls.append((entry, self))
            _init(self, *args, **kwargs)

        cls.__init__ = functools.wraps(cls.__init__)(rec)
    import causal_VAE
    import scm_world_model

    assert scm_world_model.__file__.startswith(REF) and causal_VAE.__file__.startswith(REF)
    cfg, obs = shapes.make_config("tiny", "cpu"), shapes.obs_space("tiny")
    out = {}
    for label, ctor in (("WorldModelWithSCM", scm_world_model.WorldModelWithSCM),
                        ("CausalVAE_WorldModel", causal_VAE.CausalVAE_WorldModel)):
        del calls[:]
        torch.manual_seed(0)
        model = ctor(obs, None, 0, cfg)
        where = {id(m): n for n, m in model.named_modules()}
        where.update({id(v): k for k, v in vars(model).items() if isinstance(v, tools.Optimizer)})
        rows = []
        for entry, obj in calls:
            if id(obj) not in where:  # (a piece built and dropped again)
                continue
            entry["path"] = where[id(obj)]
            if isinstance(obj, torch.nn.Module):
                entry["children"] = networks_children(obj)
                entry["numel"] = sum(p.numel() for p in obj.parameters())
            rows.append(entry)
        out[label] = {"calls": rows, "numel": sum(p.numel() for p in model.parameters())}
    for name, cls in CLASSES.items():
        cls.__init__ = originals[name]
    dst = os.path.join(HERE, "causal_construct.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print({k: [c["cls"] + "@" + c["path"] for c in v["calls"]] for k, v in out.items()}, "->", dst)


if __name__ == "__main__":
    main()
