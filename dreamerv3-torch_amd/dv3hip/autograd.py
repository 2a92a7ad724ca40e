"""torch.autograd bridge over the libdv3hip kernel pairs.

The hot path (models.WorldModel._train / ImagBehavior._train) runs an explicit, hand-derived backward and builds no
autograd graph.  Callers OUTSIDE that path -- the reference's exploration.Plan2Explore (exploration.py:40-135), its
causal world models (scm_world_model.py:129-165, 500-560; causal_VAE.py:1045-1120), anything that writes
`loss = f(head(feat).log_prob(x)); opt(loss, params)` against the public classes -- need gradients through the public
methods.  This module gives every public method a `torch.autograd.Function` whose forward AND backward are the same HIP
kernels the hot path uses (dv3hip.engine / dv3hip.ops): no ATen math re-implementation of a layer, no CPU path.

How: the engines accumulate parameter gradients into `p.grad` of the tensors in their parameter containers.  A
Function call builds a private engine over *shadow* parameters -- detached aliases of the caller's parameters that
carry a fresh zero `.grad` -- on a private Workspace (the activations must survive until backward, and the same module
may be called several times before it), runs the engine's forward, and in backward runs the engine's backward and
hands the shadows' `.grad` to autograd, which accumulates them into the real `.grad` (for parameters of a
tools.Optimizer those are views of its flat gradient bucket, so `Optimizer.__call__(loss, params)` -- tools.py:760-776
-- clips and steps them like the hot path's).

networks.py / tools.py / models.py dispatch here only when gradients are wanted (`wants_grad`); acting, logging and
the fused training path never come through this module.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import engine as E
from . import ops

F32 = torch.float32


def wants_grad(*tensors) -> bool:
    """True when autograd is recording and any of the tensors (inputs or parameters) requires a gradient."""
    if not torch.is_grad_enabled():
        return False
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            return True
    return False


def _shadow(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Detached alias of a parameter with a fresh zero .grad for the engine's backward to accumulate into."""
    if p is None:
        return None
    s = p.detach()
    s.grad = torch.zeros_like(s, memory_format=torch.contiguous_format)
    return s


def _c(t: Optional[torch.Tensor], like: Optional[torch.Tensor] = None, shape=None) -> torch.Tensor:
    """Upstream gradient as a fresh contiguous fp32 buffer the kernels may overwrite (zeros when autograd passed None)."""
    if t is None:
        return torch.zeros(shape if shape is not None else like.shape, dtype=F32, device=like.device)
    return t.to(F32).contiguous().clone()


def _rows(x: torch.Tensor) -> torch.Tensor:
    return x.reshape(-1, x.shape[-1]).to(F32).contiguous()


# ---------------------------------------------------------------------------------------------
# Linear / [Linear -> LayerNorm -> SiLU] stacks / GRU cell
# ---------------------------------------------------------------------------------------------
class LinearFn(Function):
    """y = x W^T + b (nn.Linear; networks.py:241-250 `_suff_stats_layer`, every head's mean / std layer)."""

    @staticmethod
    def forward(ctx, x, W, b):
        x2 = _rows(x)
        y = torch.empty(x2.shape[0], W.shape[0], device=x.device, dtype=F32)
        ops.gemm(x2, W.detach(), y, bias=None if b is None else b.detach())
        ctx.save_for_backward(x2, W)
        ctx.has_bias = b is not None
        ctx.lead = tuple(x.shape[:-1])
        return y.view(ctx.lead + (W.shape[0],))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        dy2 = _rows(dy)
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            ops.gemm(dy2, W.detach(), dx, transB=False)
            dx = dx.view(ctx.lead + (x2.shape[1],))
        if ctx.needs_input_grad[1]:
            dW = torch.zeros_like(W, memory_format=torch.contiguous_format)
            ops.gemm(dy2, x2, dW, transA=True, transB=False, accumulate=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(W.shape[0], device=W.device, dtype=F32)
            ops.colsum(dy2, db)
        return dx, dW, db


class TrunkFn(Function):
    """n x [Linear(no bias) -> LayerNorm(eps 1e-3) -> act] (networks.MLP.layers, networks.py:624-635; the RSSM's
    `_img_in_layers` / `_img_out_layers` / `_obs_out_layers`, networks.py:44-78) through engine.MLPEngine.
    act: the layers' activation code (ops.ACT_CODES); params = (W0, g0, b0, W1, g1, b1, ...), with g = b = None for a
    layer built with norm=False (Linear -> act; it gets no gradient for them).  The conv Functions below take their
    layers the same way."""

    @staticmethod
    def forward(ctx, x, act, *params):
        n = len(params) // 3
        x2 = _rows(x)
        layers = [E.PDenseLN(_shadow(params[3 * i]), _shadow(params[3 * i + 1]), _shadow(params[3 * i + 2]),
                             ops.act_code(act)) for i in range(n)]
        eng = E.MLPEngine("ag", E.PMLP(layers), E.Workspace(x.device))
        h, _, _ = eng.forward(x2)
        ctx.eng, ctx.x2, ctx.layers = eng, x2, layers
        ctx.lead = tuple(x.shape[:-1])
        return h.view(ctx.lead + (h.shape[-1],))

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        eng, x2 = ctx.eng, ctx.x2
        R = x2.shape[0]
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        eng.backward(x2, None, slice(0, R), dh=_c(dh.reshape(R, -1)), wgrad=any(ctx.needs_input_grad[2:]), dx1=dx)
        grads: List[Optional[torch.Tensor]] = []
        for i, L in enumerate(ctx.layers):
            for j, t in enumerate((L.W, L.g, L.b)):
                grads.append(t.grad if ctx.needs_input_grad[2 + 3 * i + j] else None)
        ctx.eng = None
        return (None if dx is None else dx.view(ctx.lead + (x2.shape[1],)), None) + tuple(grads)


class GRUFn(Function):
    """networks.GRUCell.forward (networks.py:760-768): LN(Linear(cat[x, h])) -> gates -> h'.  g = b = None: a cell built
    with norm=False, the gates on the raw Linear output."""

    @staticmethod
    def forward(ctx, x, h, W, g, b):
        x2, h2 = _rows(x), _rows(h)
        M, De = h2.shape
        pre = torch.empty(M, 3 * De, device=x.device, dtype=F32)
        ops.gemm(x2, W.detach(), pre, A2=h2)
        out = torch.empty_like(h2)
        mean = rstd = None
        if g is None:
            ops.gru_nonorm_fwd(pre, h2, out)
        else:
            mean, rstd = torch.empty(M, device=x.device), torch.empty(M, device=x.device)
            ops.gru_fwd(pre, g.detach().contiguous(), b.detach().contiguous(), h2, out, mean, rstd)
        ctx.save_for_backward(x2, h2, W, g, b, pre, mean, rstd)
        return out.view(h.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x2, h2, W, g, b, pre, mean, rstd = ctx.saved_tensors
        M, De = h2.shape
        Hd = x2.shape[1]
        wg = any(ctx.needs_input_grad[2:])
        dpre = torch.empty_like(pre)
        dh = torch.empty_like(h2)
        dg = torch.zeros_like(g) if wg and g is not None else None
        db = torch.zeros_like(b) if wg and g is not None else None
        if g is None:
            ops.gru_nonorm_bwd(_c(dout.reshape(M, De)), pre, h2, dpre, dh)
        else:
            ops.gru_bwd(_c(dout.reshape(M, De)), pre, g.detach().contiguous(), b.detach().contiguous(), h2, mean, rstd,
                        dpre, dh, dg, db)
        Wd = W.detach()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            ops.gemm(dpre, Wd[:, :Hd], dx, transB=False)
        if ctx.needs_input_grad[1]:
            ops.gemm(dpre, Wd[:, Hd:], dh, transB=False, accumulate=True)
        dW = None
        if ctx.needs_input_grad[2]:
            Ws = _shadow(W)
            E.lin_wgrad(Ws, dpre, x2, h2)
            dW = Ws.grad
        return (dx, dh if ctx.needs_input_grad[1] else None, dW, dg if ctx.needs_input_grad[3] else None,
                db if ctx.needs_input_grad[4] else None)


# ---------------------------------------------------------------------------------------------
# categorical latents
# ---------------------------------------------------------------------------------------------
class OneHotSampleFn(Function):
    """tools.OneHotDist.sample / mode (tools.py:444-460): an exact one-hot forward, the straight-through gradient
    (`+ probs - probs.detach()`, resp. `+ logits - logits.detach()` for the mode) backward."""

    @staticmethod
    def forward(ctx, logit, noise, rng, unimix, mode):
        lg = logit.detach().to(F32).contiguous()
        out = torch.empty_like(lg)
        ops.onehot_sample(lg, out, noise=None if noise is None else noise.to(F32).contiguous(), rng=rng,
                          unimix=unimix, mode=mode)
        ctx.save_for_backward(lg)
        ctx.unimix, ctx.mode = unimix, mode
        ctx.mark_non_differentiable()
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (lg,) = ctx.saved_tensors
        dl = torch.empty_like(lg)
        ops.onehot_st_bwd(lg, _c(dout.reshape(lg.shape)), dl, unimix=ctx.unimix, mode=ctx.mode)
        return dl, None, None, None, None


class OneHotEntLogpFn(Function):
    """tools.OneHotDist.entropy / log_prob per categorical group (tools.py:436-442 probabilities)."""

    @staticmethod
    def forward(ctx, logit, x, unimix, want_ent):
        lg = logit.detach().to(F32).contiguous()
        out = torch.empty(lg.shape[:-1], device=lg.device, dtype=F32)
        xs = None if x is None else x.detach().to(F32).contiguous()
        if want_ent:
            ops.onehot_ent_logp_fwd(lg, None, out, None, unimix=unimix)
        else:
            ops.onehot_ent_logp_fwd(lg, xs, None, out, unimix=unimix)
        ctx.save_for_backward(lg, xs if xs is not None else lg)
        ctx.unimix, ctx.want_ent = unimix, want_ent
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lg, xs = ctx.saved_tensors
        dl = torch.empty_like(lg)
        up = _c(dout.reshape(lg.shape[:-1]))
        if ctx.want_ent:
            ops.onehot_ent_logp_bwd(lg, None, up, None, dl, unimix=ctx.unimix)
        else:
            ops.onehot_ent_logp_bwd(lg, xs, None, up, dl, unimix=ctx.unimix)
        return dl, None, None, None


class KLLossFn(Function):
    """networks.RSSM.kl_loss (networks.py:272-290) -> loss = dyn_scale * max(dyn, free) + rep_scale * max(rep, free)
    per row; gradient through `loss` only (value / dyn / rep are logged, never optimised, by every caller)."""

    @staticmethod
    def forward(ctx, post_logit, prior_logit, free, dyn_scale, rep_scale, unimix):
        pl, ql = post_logit.detach().to(F32).contiguous(), prior_logit.detach().to(F32).contiguous()
        kl = torch.empty(pl.shape[:-2], device=pl.device, dtype=F32)
        ops.kl_fwd(pl, ql, kl, unimix=unimix)
        ctx.save_for_backward(pl, ql, kl)
        ctx.cfg = (float(free), float(dyn_scale), float(rep_scale), float(unimix))
        clipped = torch.clip(kl, min=free)
        return (dyn_scale + rep_scale) * clipped, kl.clone(), clipped, clipped.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, dvalue, ddyn, drep):
        pl, ql, kl = ctx.saved_tensors
        free, dyn_scale, rep_scale, unimix = ctx.cfg
        dp, dq = torch.empty_like(pl), torch.empty_like(ql)
        ops.kl_bwd(pl, ql, kl, dp, dq, unimix=unimix, free=free, dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=1.0)
        up = dloss.to(F32).reshape(kl.shape + (1, 1))
        return dp * up, dq * up, None, None, None, None


# ---------------------------------------------------------------------------------------------
# continuous Gaussian latents (dyn_discrete: 0)
# ---------------------------------------------------------------------------------------------
class GaussHeadFn(Function):
    """RSSM._suff_stats_layer's activations (networks.py:258-270) and the rsample / mode of get_dist(...)
    (networks.py:167-171, 228-231) on the stat layer's raw output [..., 2S] -> (mean, std, stoch)."""

    @staticmethod
    def forward(ctx, raw, eps, rng, mean_act, std_act, min_std, mode):
        r = raw.detach().to(F32).contiguous()
        S = r.shape[-1] // 2
        mk = lambda: torch.empty(r.shape[:-1] + (S,), device=r.device, dtype=F32)
        mean, std, stoch = mk(), mk(), mk()
        eps_used = None if mode else mk()
        ops.gauss_head_fwd(r, stoch, mean, std, eps=None if eps is None else eps.detach().to(F32).contiguous(), rng=rng,
                           eps_out=eps_used, mean_act=mean_act, std_act=std_act, min_std=min_std, mode=mode)
        ctx.save_for_backward(r, eps_used if eps_used is not None else r)
        ctx.cfg = (mean_act, std_act, bool(mode))
        ctx.set_materialize_grads(False)
        return mean, std, stoch

    @staticmethod
    @once_differentiable
    def backward(ctx, dmean, dstd, dstoch):
        r, eps = ctx.saved_tensors
        mean_act, std_act, mode = ctx.cfg
        S = r.shape[-1] // 2
        shp = r.shape[:-1] + (S,)
        draw = torch.empty_like(r)
        if dmean is None and dstd is None and dstoch is None:
            return draw.zero_(), None, None, None, None, None, None
        cc = lambda t: None if t is None else _c(t.reshape(shp))
        ops.gauss_head_bwd(r, draw, dstoch=cc(dstoch), dmean=cc(dmean), dstd=cc(dstd), eps=None if mode else eps,
                           mean_act=mean_act, std_act=std_act, mode=mode)
        return draw, None, None, None, None, None, None


class GaussEntropyFn(Function):
    """Entropy of Normal(mean, std) summed over the last dim (tools.NormalLatent.entropy): sum (1/2 + 1/2 ln 2 pi +
    ln std) from dv3_gauss_kl_fwd; d / d std = 1 / std, nothing reaches the mean."""

    @staticmethod
    def forward(ctx, mean, std):
        m, s = mean.detach().to(F32).contiguous(), std.detach().to(F32).contiguous()
        kl, ent = torch.empty(m.shape[:-1], device=m.device, dtype=F32), torch.empty(m.shape[:-1], device=m.device, dtype=F32)
        ops.gauss_kl_fwd(m, s, m, s, kl, ent)  # (post = prior: the entropy is the kernel's second output)
        ctx.save_for_backward(s)
        return ent

    @staticmethod
    @once_differentiable
    def backward(ctx, dent):
        (s,) = ctx.saved_tensors
        return None, dent.to(F32).unsqueeze(-1) / s


class GaussKLFn(Function):
    """networks.RSSM.kl_loss for continuous latents (networks.py:272-290 over Normal(mean, std)): gradient through
    `loss` only, as KLLossFn."""

    @staticmethod
    def forward(ctx, post_mean, post_std, prior_mean, prior_std, free, dyn_scale, rep_scale):
        t = [x.detach().to(F32).contiguous() for x in (post_mean, post_std, prior_mean, prior_std)]
        kl = torch.empty(t[0].shape[:-1], device=t[0].device, dtype=F32)
        ops.gauss_kl_fwd(*t, kl)
        ctx.save_for_backward(*t, kl)
        ctx.cfg = (float(free), float(dyn_scale), float(rep_scale))
        clipped = torch.clip(kl, min=free)
        return (dyn_scale + rep_scale) * clipped, kl.clone(), clipped, clipped.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, dvalue, ddyn, drep):
        pm, ps, qm, qs, kl = ctx.saved_tensors
        free, dyn_scale, rep_scale = ctx.cfg
        outs = [torch.empty_like(pm) for _ in range(4)]
        ops.gauss_kl_bwd(pm, ps, qm, qs, kl, dpost_mean=outs[0], dpost_std=outs[1], dprior_mean=outs[2],
                         dprior_std=outs[3], free=free, dyn_scale=dyn_scale, rep_scale=rep_scale, upstream=1.0)
        up = dloss.to(F32).reshape(kl.shape + (1,))
        return tuple(o * up for o in outs) + (None, None, None)


# ---------------------------------------------------------------------------------------------
# RSSM.observe: the whole scan as one node (engine.RSSMEngine.observe_fwd / observe_bwd)
# ---------------------------------------------------------------------------------------------
def rssm_param_list(P: E.PRSSM) -> List[torch.Tensor]:
    return [P.W0, P.img_in.W, P.img_in.g, P.img_in.b, P.gru.W, P.gru.g, P.gru.b, P.img_out.W, P.img_out.g,
            P.img_out.b, P.obs_out.W, P.obs_out.g, P.obs_out.b, P.ims.W, P.ims.b, P.obs.W, P.obs.b]


def _rssm_shadow(params: Sequence[torch.Tensor], act: int = 1) -> E.PRSSM:
    s = [_shadow(p) for p in params]
    return E.PRSSM(s[0], E.PDenseLN(*s[1:4], act), E.PDenseLN(*s[4:7]), E.PDenseLN(*s[7:10], act),
                   E.PDenseLN(*s[10:13], act), E.PLin(*s[13:15]), E.PLin(*s[15:17]))


def _observe_forward(ctx, embed_tm, action_tm, first_tm, q_prior, q_post, rng, dims, params, keys):
    """Forward of both observe nodes: a private engine over shadow parameters runs observe_fwd, ctx keeps it for the
    backward, and the outputs are clones of the engine's buffers `keys`."""
    dims = dict(dims)
    P = _rssm_shadow(params, ops.act_code(dims.pop("act", True)))  # (dims["act"]: the three dense blocks' activation)
    eng = E.RSSMEngine(P, E.Workspace(embed_tm.device), **dims)
    f32 = lambda x: x.detach().to(F32).contiguous()
    out = eng.observe_fwd(f32(embed_tm), f32(action_tm), f32(first_tm), q_prior=q_prior, q_post=q_post, rng=rng)
    ctx.eng, ctx.P, ctx.out = eng, P, out
    ctx.set_materialize_grads(False)
    return tuple(out[k].clone() for k in keys)


def _observe_backward_tail(ctx, side, dembed):
    """Behind observe_bwd (which returned `side`): the gradients of both observe nodes' 7 inputs + 17 parameters."""
    side.join()
    grads = [p.grad if ctx.needs_input_grad[7 + i] else None for i, p in enumerate(rssm_param_list(ctx.P))]
    ctx.eng = ctx.out = None
    return (dembed if ctx.needs_input_grad[0] else None, None, None, None, None, None, None) + tuple(grads)


class ObserveFn(Function):
    """networks.RSSM.observe (networks.py:127-143) on time-major inputs.  Outputs (post_stoch, post_logit, deter,
    prior_stoch, prior_logit), each [T,B,...]; gradients flow to `embed` and the 17 RSSM parameters (the action
    and the reset flags are data)."""

    KEYS = ("post_stoch", "post_logit", "deter", "prior_stoch", "prior_logit")  # observe_fwd's names of the outputs

    @staticmethod
    def forward(ctx, embed_tm, action_tm, first_tm, q_prior, q_post, rng, dims, *params):
        return _observe_forward(ctx, embed_tm, action_tm, first_tm, q_prior, q_post, rng, dims, params, ObserveFn.KEYS)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_ps, d_pl, d_dt, d_qs, d_ql):
        eng, out = ctx.eng, ctx.out
        T, B, S, D, De = eng.T, eng.B, eng.S, eng.D, eng.De
        like = out["deter"]
        dpl = _c(d_pl, shape=(T, B, S, D), like=like)
        dql = _c(d_ql, shape=(T, B, S, D), like=like)
        if d_qs is not None:  # the prior sample's straight-through path into its logits
            ops.onehot_st_bwd(out["prior_logit"], _c(d_qs.reshape(T, B, S, D)), dql, unimix=eng.unimix, accumulate=True)
        gs = _c(None if d_ps is None else d_ps.reshape(T, B, S * D), shape=(T, B, S * D), like=like)
        gd = _c(d_dt, shape=(T, B, De), like=like)
        dembed = torch.empty(T, B, eng.E, device=like.device, dtype=F32)
        return _observe_backward_tail(ctx, eng.observe_bwd(dpl, dql, gs, gd, dembed), dembed)


class ObserveGaussFn(Function):
    """ObserveFn for continuous latents.  Outputs (post_stoch, post_mean, post_std, deter, prior_stoch, prior_mean,
    prior_std), each [T,B,...]; eps_prior / eps_post [T,B,S] ~ N(0,1) or the rng stream."""

    KEYS = ("post_stoch", "post_mean", "post_std", "deter", "prior_stoch", "prior_mean", "prior_std")

    @staticmethod
    def forward(ctx, embed_tm, action_tm, first_tm, eps_prior, eps_post, rng, dims, *params):
        return _observe_forward(ctx, embed_tm, action_tm, first_tm, eps_prior, eps_post, rng, dims, params,
                                ObserveGaussFn.KEYS)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_ps, d_pm, d_psd, d_dt, d_qs, d_qm, d_qsd):
        eng, out = ctx.eng, ctx.out
        T, B, S, De = eng.T, eng.B, eng.S, eng.De
        like = out["deter"]
        cc = lambda t: None if t is None else _c(t.reshape(T, B, S))
        gs = _c(d_ps, shape=(T, B, S), like=like)
        gd = _c(d_dt, shape=(T, B, De), like=like)
        dembed = torch.empty(T, B, eng.E, device=like.device, dtype=F32)
        side = eng.observe_bwd((cc(d_pm), cc(d_psd)), (cc(d_qm), cc(d_qsd), cc(d_qs)), gs, gd, dembed)
        return _observe_backward_tail(ctx, side, dembed)


# ---------------------------------------------------------------------------------------------
# conv stacks
# ---------------------------------------------------------------------------------------------
class ConvEncoderFn(Function):
    """networks.ConvEncoder.forward (networks.py:486-496) on x = image - 0.5 [N,H,W,C]; act: the layers' activation
    code; params = (W, g, b) per layer.  The image itself gets no gradient (it is data for every caller)."""

    @staticmethod
    def forward(ctx, x, size, act, *params):
        layers = [E.PConvLayer(_shadow(params[3 * i]), _shadow(params[3 * i + 1]), _shadow(params[3 * i + 2]),
                               act=ops.act_code(act)) for i in range(len(params) // 3)]
        eng = E.ConvEncoderEngine(layers, E.Workspace(x.device), size=size)
        emb = eng.forward(x_f32=x.detach().to(F32).contiguous(), keep=True)
        ctx.eng, ctx.layers = eng, layers
        return emb.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, demb):
        ctx.eng.backward(_c(demb))
        grads = []
        for i, L in enumerate(ctx.layers):
            for j, t in enumerate((L.W, L.g, L.b)):
                grads.append(t.grad if ctx.needs_input_grad[3 + 3 * i + j] else None)
        ctx.eng = None
        return (None, None, None) + tuple(grads)


class ConvDecoderFn(Function):
    """networks.ConvDecoder.forward (networks.py:568-585): feat [R,F] -> mean image [R,64,64,3] (+0.5).
    act: the layers' activation code; params = (lin.W, lin.b, W0, g0, b0, ..., W_last, bias_last)."""

    @staticmethod
    def forward(ctx, feat, minres, act, *params):
        lin = E.PLin(_shadow(params[0]), _shadow(params[1]))
        rest = params[2:]
        n_ln = (len(rest) - 2) // 3
        layers = [E.PConvLayer(_shadow(rest[3 * i]), _shadow(rest[3 * i + 1]), _shadow(rest[3 * i + 2]),
                               act=ops.act_code(act)) for i in range(n_ln)]
        layers.append(E.PConvLayer(_shadow(rest[-2]), None, None, _shadow(rest[-1])))
        eng = E.ConvDecoderEngine(lin, layers, E.Workspace(feat.device), minres=minres)
        x = _rows(feat)
        F_ = x.shape[1]
        k1 = max(32, (F_ // 2) // 32 * 32) if F_ >= 64 else F_ // 2  # two K segments, as get_feat's [stoch | deter]
        x1, x2 = x[:, :k1].contiguous(), x[:, k1:].contiguous()
        rec = eng.forward(x1, x2)
        ctx.eng, ctx.lin, ctx.layers, ctx.k1, ctx.F = eng, lin, layers, k1, F_
        return rec.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, drec):
        R = drec.shape[0]
        dx1 = torch.empty(R, ctx.k1, device=drec.device, dtype=F32)
        dx2 = torch.empty(R, ctx.F - ctx.k1, device=drec.device, dtype=F32)
        ctx.eng.backward(_c(drec), dx1, dx2)
        flat = [ctx.lin.W, ctx.lin.b]
        for L in ctx.layers[:-1]:
            flat += [L.W, L.g, L.b]
        flat += [ctx.layers[-1].W, ctx.layers[-1].bias]
        grads = [t.grad if ctx.needs_input_grad[3 + i] else None for i, t in enumerate(flat)]
        ctx.eng = None
        return (torch.cat([dx1, dx2], 1) if ctx.needs_input_grad[0] else None, None, None) + tuple(grads)


# ---------------------------------------------------------------------------------------------
# distribution heads
# ---------------------------------------------------------------------------------------------
class DiscModeFn(Function):
    """tools.DiscDist.mean / mode (tools.py:475-486): symexp(sum softmax(l) * buckets)."""

    @staticmethod
    def forward(ctx, logits):
        lg = logits.detach().to(F32).contiguous()
        out = torch.empty(lg.shape[:-1] + (1,), device=lg.device, dtype=F32)
        ops.disc_mode_fwd(lg, out)
        ctx.save_for_backward(lg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (lg,) = ctx.saved_tensors
        dl = torch.empty_like(lg)
        ops.disc_mode_bwd(lg, _c(dout.reshape(lg.shape[:-1])), dl)
        return dl


class DiscLogProbFn(Function):
    """tools.DiscDist.log_prob (tools.py:488-517): two-hot cross entropy against symlog(x)."""

    @staticmethod
    def forward(ctx, logits, x):
        lg = logits.detach().to(F32).contiguous()
        xs = x.detach().to(F32).contiguous()
        out = torch.empty(lg.shape[:-1], device=lg.device, dtype=F32)
        ops.disc_logprob_fwd(lg, xs, out)
        ctx.save_for_backward(lg, xs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lg, xs = ctx.saved_tensors
        dl = torch.empty_like(lg)
        ops.disc_logprob_bwd(lg, xs, _c(dout.reshape(lg.shape[:-1])), dl)
        return dl, None


class BernoulliLogProbFn(Function):
    """tools.Bernoulli.log_prob (tools.py:620-628) elementwise on logits."""

    @staticmethod
    def forward(ctx, logit, x):
        lg = logit.detach().to(F32).contiguous()
        xs = x.detach().to(F32).contiguous().reshape(lg.shape)
        out = torch.empty_like(lg)
        ops.bernoulli_logprob_fwd(lg, xs, out)
        ctx.save_for_backward(lg, xs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lg, xs = ctx.saved_tensors
        dl = torch.empty_like(lg)
        ops.bernoulli_logprob_bwd(lg, xs, _c(dout.reshape(lg.shape)), dl)
        return dl, None


class SymlogMSEFn(Function):
    """tools.SymlogDist.log_prob (tools.py:556-572, mse / sum): -sum (mode - symlog(x))^2 with the 1e-8 cut."""

    @staticmethod
    def forward(ctx, mode, x):
        m = mode.detach().to(F32).contiguous()
        xs = x.detach().to(F32).contiguous()
        loss = torch.empty(m.shape[:-1], device=m.device, dtype=F32)
        dmode = torch.empty_like(m)
        ops.symlog_mse(m, xs, loss, dmode, upstream=1.0)
        ctx.save_for_backward(dmode)
        return -loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (dmode,) = ctx.saved_tensors
        return dmode * (-dout.to(F32)).unsqueeze(-1), None


class NormalFn(Function):
    """The continuous actor's Normal(tanh(mean), (max-min) sigmoid(std + 2) + min) (networks.py:693-700) under
    tools.ContDist (tools.py:575-601).  kind: "sample" (rsample from eps, absmax 1 rescale detached), "entropy",
    "logp" (of a given action, treated as a constant)."""

    @staticmethod
    def forward(ctx, mean_raw, std_raw, aux, kind, min_std, max_std):
        mr, sr = mean_raw.detach().to(F32).contiguous(), std_raw.detach().to(F32).contiguous()
        ax = None if aux is None else aux.detach().to(F32).contiguous()
        lead = mr.shape[:-1]
        if kind == "sample":
            out = torch.empty_like(mr)
            ops.actor_normal_fwd(mr, sr, ax, out, None, min_std=min_std, max_std=max_std)
        elif kind == "entropy":
            out = torch.empty(lead, device=mr.device, dtype=F32)
            ops.actor_normal_fwd(mr, sr, None, None, out, min_std=min_std, max_std=max_std)
        else:
            out = torch.empty(lead, device=mr.device, dtype=F32)
            ops.actor_normal_logp(mr, sr, ax, out, min_std=min_std, max_std=max_std)
        ctx.save_for_backward(mr, sr, ax if ax is not None else mr, out)
        ctx.kind, ctx.stds = kind, (min_std, max_std)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        mr, sr, ax, out = ctx.saved_tensors
        dm, ds = torch.empty_like(mr), torch.empty_like(sr)
        lo, hi = ctx.stds
        up = _c(dout.reshape(out.shape))
        if ctx.kind == "sample":
            ops.actor_normal_bwd(mr, sr, dm, ds, eps=ax, action=out, daction=up, min_std=lo, max_std=hi)
        elif ctx.kind == "entropy":
            ops.actor_normal_bwd(mr, sr, dm, ds, dent=up, min_std=lo, max_std=hi)
        else:
            ops.actor_normal_bwd(mr, sr, dm, ds, action=ax, dlogp=up, min_std=lo, max_std=hi)
        return dm, ds, None, None, None, None


class TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        xs = x.detach().to(F32).contiguous()
        y = torch.empty_like(xs)
        ops.tanh_fwd(xs, y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        ops.tanh_bwd(y, _c(dy.reshape(y.shape)), dx)
        return dx
