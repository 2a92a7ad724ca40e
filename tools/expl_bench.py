#!/usr/bin/env python3
"""Device time of one Plan2Explore exploration update (ensemble regression + Adam, exploration behaviour on the
disagreement reward) at cfg 2 -- categorical latents (`cfg2`) or continuous ones (`cfg2_gauss`, dyn_discrete: 0) --
with the stock exploration settings of configs.yaml, MI355X only:

  * autograd route  -- exploration.Plan2Explore.train (expl_fused False: the parent path), eager;
  * fused           -- train_fwd_bwd + train_opt on the member-batched ensemble kernels, eager and as a hipGraph replay;
  * a per-kernel table (HIP events, by shape) of the fused update with the achieved TFLOP/s of the batched GEMMs
    against the fp32 matrix peak, and the libdv3hip launch counts of both routes (ATen launches of the autograd
    route -- stack, std, mean, log, autograd's accumulations -- are not counted: the figure is a lower bound).

Both routes run in this process on the same weights, alternating, after warm-up; times are medians of device-event
intervals around whole updates.  The EAGER figures therefore include the host's launch gaps (a route that issues many
small launches is bounded by the host, not by the device); the replay figure is device time and covers the fused route
only (the autograd route cannot be captured).

    python tools/expl_bench.py [cfg2 | cfg2_gauss] [--json out.json] [--no-replay]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dreamerv3-torch_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import helpers as Hh  # noqa: E402
from tests.golden import common, gauss_common  # noqa: E402

PEAK_TFLOPS = 157.3  # fp32 matrix peak (README)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import exploration
    from dv3hip import ops

    if not torch.cuda.is_available():
        raise SystemExit("expl_bench needs a GPU")
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_json]
    name = args[0] if args else "cfg2"
    # (continuous latents: `stoch` wide states and 2 * stoch wide stat layers, gauss_common's weight table)
    weights = None if common.SHAPES[name]["discrete"] else gauss_common.make_weights(name)
    cfg, wm, _ = Hh.build_models(name, weights=weights)
    cfg.expl_behavior = "plan2explore"
    torch.manual_seed(0)
    p2e = exploration.Plan2Explore(cfg, wm, lambda f, st, a: wm.heads["reward"](f).mean()).cuda()
    p2e.requires_grad_(False)
    data = {k: torch.from_numpy(v).cuda() for k, v in common.make_batch(name).items()}
    post, context, _ = wm._train(data)
    post = {k: v.clone() for k, v in post.items()}

    def autograd_update():
        return p2e.train(post, context, data)[-1]

    def fused_update():
        p2e.train_fwd_bwd(post, context, data)
        return p2e.train_opt(allreduce=False)[-1]

    for _ in range(2):  # warm: code objects, workspaces, the bucket
        autograd_update()
        fused_update()
    torch.cuda.synchronize()
    t_a, t_f = [], []
    for _ in range(7):  # alternating
        t_a.append(event_ms(autograd_update))
        t_f.append(event_ms(fused_update))
    res = dict(config=name, dyn_discrete=cfg.dyn_discrete, disag_target=cfg.disag_target, disag_models=cfg.disag_models, disag_layers=cfg.disag_layers, disag_units=cfg.disag_units,
               autograd_eager_ms=float(np.median(t_a)), fused_eager_ms=float(np.median(t_f)),
               autograd_eager_all_ms=t_a, fused_eager_all_ms=t_f)
    ops.PROFILE.by_shape = False
    ops.PROFILE.start()
    autograd_update()
    res["autograd_libdv3hip_launches"] = sum(v["launches"] for v in ops.PROFILE.stop().values())
    ops.PROFILE.by_shape = True
    ops.PROFILE.start()
    fused_update()
    prof = ops.PROFILE.stop()
    ops.PROFILE.by_shape = False
    res["fused_launches"] = sum(v["launches"] for v in prof.values())
    ens = {k: v for k, v in prof.items() if k.startswith(("ens_", "dv3_ens_"))}
    res["fused_ensemble_launches"] = sum(v["launches"] for v in ens.values())
    res["fused_ensemble_ms"] = sum(v["ms"] for v in ens.values())
    res["by_kernel"] = {k: dict(v, tflops=v["flops"] / max(v["ms"], 1e-9) / 1e9,
                                peak_share=v["flops"] / max(v["ms"], 1e-9) / 1e9 / PEAK_TFLOPS)
                        for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
    print("(eager figures include host launch gaps; the replay figure is device time, fused route only)")
    print(f"{name}: exploration update  autograd route {res['autograd_eager_ms']:.2f} ms eager "
          f"({res['autograd_libdv3hip_launches']} libdv3hip launches + ATen's)   fused {res['fused_eager_ms']:.2f} ms eager "
          f"({res['fused_launches']} launches, {res['fused_ensemble_launches']} of them the ensemble's = "
          f"{res['fused_ensemble_ms']:.2f} ms)")
    for k, v in list(res["by_kernel"].items())[:30]:
        print(f"  {v['ms']:8.3f} ms  n={v['launches']:4d}  {v['ms'] * 1e3 / v['launches']:8.1f} us/launch  "
              f"{v['tflops']:6.1f} TF/s ({100 * v['peak_share']:4.1f} %)  {k}")
    if out_json:
        json.dump(res, open(out_json, "w"), indent=1)
    if "--no-replay" not in sys.argv:
        st = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                fused_update()
        g.replay()
        torch.cuda.synchronize()
        res["fused_replay_all_ms"] = [event_ms(g.replay) for _ in range(10)]
        res["fused_replay_ms"] = float(np.median(res["fused_replay_all_ms"]))
        print(f"  fused, hipGraph replay: {res['fused_replay_ms']:.2f} ms")
        if out_json:
            json.dump(res, open(out_json, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, (dict, list))}))


if __name__ == "__main__":
    main()
