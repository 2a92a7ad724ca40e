"""Float64 parity of the row-fused kernels of the imagination step (csrc/fusedops.hip) and of the column-sum /
statistics helpers, at the edges of their host dispatch.

Every comparison is one HIP kernel, called through dv3hip.ops (or through ctypes where the wrapper cannot express the
call), against a plain float64 PyTorch expression of the same operation on the CPU.  Inputs are seeded fp32 tensors
cast to float64; every reference function takes `dt`, so that test_fp32_oracle_error_is_under_half_the_bar can
evaluate it in fp32 on the CPU: that number is measured against the reference, never against a kernel.

  A  onehot_linear_ln         vec kernel NV4 = 1..4 and the generic kernel (N = 1, 255, 257, 260, 1280); the fall-back
                              to the generic kernel at N = 256 by each leading dimension = 1 (mod 4); S = 1 .. 64 (the
                              second MAXB batch at S = 33, 64); idx all 0 / all D - 1; the dense tail A2 = 0 .. 5 as a
                              column window; base none / separate / aliasing pre; y = None; statistics None; act codes
                              0, 1 and a runtime code; one row above each grid cap; the LayerNorm row kinds of
                              tests/test_ln_gru_f64_gpu.py; `pre` EXACT on integers in both kernels.
  B  onehot_sample_linear_ln  S = 1, 7, 31, 32 x N = 256 .. 1024; next_first all 0 / all 1 / mixed; mode, injected
                              noise, forced + flips, idx = None; randn / wide / edge logits; one row past the 32768
                              workgroup cap; every output against float64 evaluated on the kernel's own draw.
  C  actor_head               U at the edges of NV = 1, 4, 8, 16 x A over a full batch, a remainder and a second batch
                              of OB = 12 and OB = 6 outputs; every rotation; M = 1; the second trip of the row loop;
                              odd column windows; both actors, saturated heads, ties, forced / flips, Philox noise.
  D  transpose2d(_many), onehot_to_idx   bit-exact.
  E  gemm_sample              the direct kernel at 4 waves (K = 3 .. 49) and 8 waves (K = 497, 512); l16 + sample at the
                              smallest output that selects it and the same size with l16_ok false (profile keys
                              asserted); M = 1 .. 100 x N = 64 .. 192; bias None, mode, forced / flips, idx None;
                              LayerNorm on load (K = 4, 36, 512, a column window, the row kinds, statistics None);
                              the [A | A2] seam at K1 = 16, 32, 48 through ctypes; logits EXACT on integers.
  G  colsum (slab kernel with and without atomics, the narrow kernel from R = 4096 at N <= 32 and past its grid
     cap; EXACT on integers), colsum_grouped (1 and 48 items through ctypes), tensorstats(_multi) (aligned and
     4-byte-aligned bases, n = 1 .. 1025, constant and 1e4 + randn data), quantile2_ema (register cache on / off,
     q = 0 / 1 / q0 == q1, infinities, equal / negative / denormal values, alpha 0 and 1; torch.quantile's fp32 result
     to the last ulp of the interpolation, as tests/test_kernels_gpu.py holds it).

Bars: 1e-4 * max(1, max |ref|) (TOL of tests/test_kernels_gpu.py); rstd of the spiked rows against its own maximum
(floor 0, as tests/test_ln_gru_f64_gpu.py).  Draws: the kernel's class must equal the float64 argmax of p_hat / q on
every row whose float64 top-two scores are more than 1e-5 relative apart (the excluded share is asserted <= 1e-3; an
EXACT float64 tie is not excluded: the lowest index must win); everything downstream of a draw is compared with
float64 evaluated on the kernel's own draw.  Rejections return DV3_ERR_ARG with every output still at its sentinel.
No bar is widened: the worst fp32-oracle error / bar per group is asserted under 0.5 (CPU test below; measured: A 0.027,
B 0.013, C 0.027, E 0.030, G 0.009).
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.test_ln_gru_f64_gpu import rows_of
from tests.test_row_kernels_f64_gpu import TIE_CAP, TIE_REL, cat_logits, check, dev, gen

TOL = 1e-4
EPS = 1e-3  # every LayerNorm on the path (kLnEps)
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
PAD = 7777.0
ERR_ARG = 10001  # DV3_ERR_ARG of include/dv3hip.h
LN_KINDS = ["randn", "offset", "tiny", "spike", "const"]
RT_ACT = "Tanh"  # the runtime-code activation of these tests (code 5)
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def lib():
    from dv3hip import _lib

    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def act_fn(z, act):
    if act in (False, 0):
        return z
    if act in (True, 1):
        return F.silu(z)
    assert act == RT_ACT
    return torch.tanh(z)


def ln_act(pre, gamma, beta, act):
    mean = pre.mean(-1, keepdim=True)
    d = pre - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS)
    return act_fn(d * rstd * gamma + beta, act), mean[:, 0], rstd[:, 0]


def seed_of(c, salt=0):
    """A seed that depends on the case alone (not on its position in a list or on the process)."""
    return zlib.crc32(repr(sorted(c.items())).encode()) % 1000003 + salt


def ints(shape, g):
    return torch.randint(-3, 4, tuple(shape), generator=g).float()


def place(t, extra=0, off=0, v=PAD):
    """-> (buffer [R, W + extra] of v, its column window [off, off + W) holding t): ld = W + extra."""
    R, W = t.shape
    assert off <= extra
    buf = torch.full((R, W + extra), v, device="cuda")
    win = buf[:, off:off + W]
    win.copy_(t)
    return buf, win


def outside_untouched(buf, off, W, v=PAD):
    o = torch.cat([buf[:, :off], buf[:, off + W:]], 1)
    return bool(torch.isnan(o).all()) if v != v else bool((o == v).all())


def exact(got, ref, what):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int((got != ref).sum())
    print(f"{what}: exact" if bad == 0 else f"{what}: {bad} of {ref.numel()} differ")
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"


def ratio(r32, r64, floor=1.0):
    """fp32 oracle error as a fraction of the bar check() applies."""
    r64 = r64.double()
    if not r64.numel():
        return 0.0
    return (r32.double() - r64).abs().max().item() / (TOL * max(floor, r64.abs().max().item()))


# ================================================================================================ A. onehot_linear_ln
def OL(M, S, D, N, A2=3, base="sep", y=True, stats=True, act=True, idx="rand", odd=None, kind="randn"):
    """odd: the one operand (w / pre / base / y) whose leading dimension is = 1 (mod 4); all others are windows at
    column 1 of a buffer 4 wider (ld = 0 mod 4 where N is: the vec kernel must take an address that is only 4-byte
    aligned).  kind: the LayerNorm row kind, carried by `base` (the gathered weights are then 1e-3 randn; 0 for const)."""
    return dict(M=M, S=S, D=D, N=N, A2=A2, base=base, y=y, stats=stats, act=act, idx=idx, odd=odd, kind=kind)


def ol_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if v is not None)


OL_WIDTHS = [OL(3, 5, 7, N) for N in (256, 512, 768, 1024, 1, 255, 257, 260, 1280)]
OL_FALLBACK = [OL(3, 5, 7, 256, odd=o) for o in ("w", "pre", "base", "y")]
OL_GROUPS = [OL(3, S, D, N) for N in (256, 20) for S, D in ((1, 32), (4, 7), (5, 1), (32, 32), (33, 7), (64, 32))]
OL_IDX = [OL(3, 33, 7, N, idx=i) for N in (256, 20) for i in ("zero", "last")]
OL_TAIL = [OL(3, 5, 7, N, A2=a) for N in (512, 257) for a in (0, 1, 4, 5)]
OL_FORMS = ([OL(3, 5, 7, N, **kw) for N in (768, 260) for kw in
             (dict(base=None), dict(base="alias"), dict(y=False), dict(stats=False), dict(act=False), dict(act=RT_ACT),
              dict(act=RT_ACT, base="alias", stats=False))])
OL_ROWS = [OL(1, 5, 7, 256), OL(1, 5, 7, 255), OL(32768 + 5, 4, 7, 256), OL(16384 + 3, 4, 7, 20)]
OL_KINDS = [OL(5, 4, 7, N, kind=k) for N in (256, 255) for k in LN_KINDS[1:]]
OL_CASES = OL_WIDTHS + OL_FALLBACK + OL_GROUPS + OL_IDX + OL_TAIL + OL_FORMS + OL_ROWS + OL_KINDS


def ol_ld(c, name):
    """Leading dimension of operand name (w / pre / base / y) of case c: = 1 (mod 4) for the case's odd operand, else
    the next multiple of 4 above N."""
    N = c["N"]
    return N + ((((1 - N) % 4) or 4) if c["odd"] == name else (((-N) % 4) or 4))


def ol_inputs(c, mode):
    """mode "randn" | "int" -> CPU fp32 dict(idx, WT, x2, base, gamma, beta)."""
    M, S, D, N, A2 = c["M"], c["S"], c["D"], c["N"], c["A2"]
    g = gen(seed_of(c, 977 if mode == "int" else 0))
    if c["idx"] == "rand":
        idx = torch.randint(0, D, (M, S), generator=g)
    else:
        idx = torch.full((M, S), 0 if c["idx"] == "zero" else D - 1)
    draw = (lambda *s: ints(s, g)) if mode == "int" else (lambda *s: torch.randn(*s, generator=g))
    WT = draw(S * D + A2, N)
    x2 = draw(M, A2) if A2 else None
    base = draw(M, N) if c["base"] else None
    if c["kind"] != "randn" and mode != "int":
        base = rows_of(M, N, c["kind"], g)
        WT = WT * (0.0 if c["kind"] == "const" else 1e-3)
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    return dict(idx=idx.int(), WT=WT, x2=x2, base=base, gamma=gamma, beta=beta)


def ol_ref(t, c, dt=F64, idx=None):
    """-> dict(pre, y, mean, rstd): base + the S gathered rows of WT (+ x2 @ WT[S*D:]), LayerNorm, activation."""
    S, D = c["S"], c["D"]
    idx = (t["idx"] if idx is None else idx).long()
    W = t["WT"].to(dt)
    pre = t["base"].to(dt).clone() if t["base"] is not None else torch.zeros(idx.shape[0], W.shape[1], dtype=dt)
    for s in range(S):
        pre += W[s * D + idx[:, s]]
    if t["x2"] is not None:
        pre += t["x2"].to(dt) @ W[S * D:]
    y, mean, rstd = ln_act(pre, t["gamma"].to(dt), t["beta"].to(dt), c["act"])
    return dict(pre=pre, y=y, mean=mean, rstd=rstd)


def ol_floor(c):
    return 0.0 if c["kind"] == "spike" else 1.0


def ol_ratio(c):
    t = ol_inputs(c, "randn")
    a, b = ol_ref(t, c, F32), ol_ref(t, c, F64)
    return max(ratio(a[k], b[k], ol_floor(c) if k == "rstd" else 1.0) for k in a)


def run_ol(ops, c, mode):
    M, N = c["M"], c["N"]
    t = ol_inputs(c, mode)
    ref = ol_ref(t, c)
    what = f"onehot_linear_ln {ol_id(c)} {mode}"
    ex = lambda name: ol_ld(c, name) - N
    for name in ("w", "pre", "base", "y"):  # the leading dimensions this case claims
        assert (N + ex(name)) % 4 == (1 if c["odd"] == name else 0), (name, N + ex(name))
    _, WT = place(t["WT"], ex("w"), 1)
    x2 = place(t["x2"], 3, 2)[1] if t["x2"] is not None else None
    if c["base"] == "alias":
        pbuf, pre = place(t["base"], ex("pre"), 1, NAN)
        base = pre
    else:
        pbuf, pre = place(torch.full((M, N), NAN), ex("pre"), 1, NAN)
        base = place(t["base"], ex("base"), 1)[1] if t["base"] is not None else None
    ybuf, y = place(torch.full((M, N), NAN), ex("y"), 1, NAN) if c["y"] else (None, None)
    mean, rstd = ((torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")) if c["y"] and c["stats"]
                  else (None, None))
    gamma, beta = (dev(t["gamma"]), dev(t["beta"])) if c["y"] else (None, None)
    ops.onehot_linear_ln(dev(t["idx"]), c["D"], WT, pre, x2=x2, base=base, gamma=gamma, beta=beta, y=y, mean=mean,
                         rstd=rstd, act=c["act"])
    assert bool(torch.isnan(pbuf[:, :1]).all()) and bool(torch.isnan(pbuf[:, 1 + N:]).all()), what + ": wrote outside pre"
    if mode == "int":
        assert 3 + 3 * c["S"] + 9 * c["A2"] < 2 ** 23  # every partial sum is an integer fp32 holds
        return exact(pre, ref["pre"], what + " pre")
    check(pre, ref["pre"], what=what + " pre")
    if c["y"]:
        assert bool(torch.isnan(ybuf[:, :1]).all()) and bool(torch.isnan(ybuf[:, 1 + N:]).all()), what + ": wrote outside y"
        check(y, ref["y"], what=what + " y")
        if c["stats"]:
            check(mean, ref["mean"], what=what + " mean")
            check(rstd, ref["rstd"], what=what + " rstd", floor=ol_floor(c))


@gpu
@pytest.mark.parametrize("c", OL_CASES, ids=ol_id)
def test_onehot_linear_ln(ops, c):
    run_ol(ops, c, "randn")
    run_ol(ops, c, "int")


@gpu
def test_onehot_linear_ln_rejections():
    """S = 65, N > ldw / ldpre, an unknown activation code, y without gamma: DV3_ERR_ARG and pre still NaN."""
    M, S, D, N = 3, 4, 7, 256
    g = gen(11)
    idx, WT = dev(torch.randint(0, D, (M, 65), generator=g).int()), dev(torch.randn(65 * D, N, generator=g))
    pre, y = torch.full((M, N), NAN, device="cuda"), torch.full((M, N), NAN, device="cuda")
    gm = dev(torch.ones(N))

    def call(S=S, ldw=N, ldpre=N, act=1, gamma=gm, yy=y):
        rc = lib().dv3_onehot_linear_ln_fwd(ptr(idx), S, D, 0, 0, 0, ptr(WT), ldw, 0, 0, ptr(pre), ldpre, ptr(gamma), ptr(gm),
                                            ptr(yy), N, 0, 0, M, N, act, stream())
        torch.cuda.synchronize()
        return rc

    for what, kw in (("S = 65", dict(S=65)), ("ldw < N", dict(ldw=N - 1)), ("ldpre < N", dict(ldpre=N - 1)),
                     ("act code 7", dict(act=7)), ("y without gamma", dict(gamma=None))):
        assert call(**kw) == ERR_ARG, what
        assert bool(torch.isnan(pre).all()) and bool(torch.isnan(y).all()), what + ": an output was written"
    assert call() == 0 and bool(torch.isfinite(pre).all())


# ======================================================================================= B. onehot_sample_linear_ln
U_MIX = 0.01


def SL(M, S, N, A2=3, first="mixed", smp="noise", logits="randn", idx=True, act=True, kind="randn"):
    """smp: "noise" (injected Exp(1)) | "mode" | "forced".  kind != randn: S = 1 and WT's rows are that LayerNorm row
    kind (pre = one gathered row)."""
    return dict(M=M, S=S, N=N, A2=A2, first=first, smp=smp, logits=logits, idx=idx, act=act, kind=kind)


SL_CASES = ([SL(5, S, N, A2=(0 if (S + N // 256) % 2 else 3)) for S in (1, 7, 31, 32) for N in (256, 512, 768, 1024)] +
            [SL(1, 7, 512), SL(32768 + 3, 1, 256, A2=0)] +
            [SL(5, 7, 256, first=f) for f in ("zero", "one")] +
            [SL(5, 31, 512, smp="mode"), SL(5, 32, 768, smp="forced"), SL(5, 7, 256, idx=False), SL(5, 7, 256, act=False)] +
            [SL(5, 7, 512, logits=k, smp=s) for k in ("wide", "edge") for s in ("noise", "mode")] +
            [SL(5, 1, 256, A2=0, kind=k) for k in LN_KINDS[1:]])


def sl_inputs(c):
    M, S, N, A2 = c["M"], c["S"], c["N"], c["A2"]
    g = gen(seed_of(c, 1))
    logit = cat_logits(M * S, 32, c["logits"], g).reshape(M, S, 32)
    q = torch.empty(M, S, 32).exponential_(generator=g)
    first = {"zero": torch.zeros(M), "one": torch.ones(M), "mixed": (torch.arange(M) % 3 == 1).float()}[c["first"]]
    init_idx = torch.randint(0, 32, (S,), generator=g)
    forced = torch.randint(0, 32, (M, S), generator=g) if c["smp"] == "forced" else None
    WT = torch.randn(S * 32 + A2, N, generator=g)
    if c["kind"] != "randn":
        WT = rows_of(32, N, c["kind"], g)
    x2 = torch.randn(M, A2, generator=g) if A2 else None
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    return dict(logit=logit, q=q, first=first, init_idx=init_idx.int(), init=F.one_hot(init_idx, 32).float(),
                forced=forced, WT=WT, x2=x2, base=None, gamma=gamma, beta=beta)


def draw_ref(logit, q, unimix, dt=F64):
    """[R, D] -> (class [R], excluded [R]): argmax of p_hat / q (q None: the mode), lowest index on an exact tie;
    excluded = top-two within TIE_REL relative but not exactly equal."""
    D = logit.shape[-1]
    p = F.softmax(logit.to(dt), -1) * (1 - unimix) + unimix / D
    s = p if q is None else p / q.to(dt)
    idx = s.argmax(-1)
    if D < 2:
        return idx, torch.zeros(logit.shape[0], dtype=torch.bool)
    top = s.topk(2, -1).values
    return idx, ((top[:, 0] - top[:, 1]) < TIE_REL * top[:, 0]) & (top[:, 0] != top[:, 1])


def sl_down(t, c, kidx, dt=F64):
    """Everything downstream of the draw kidx [M, S]."""
    m = t["first"].to(dt)[:, None, None]
    onehot = F.one_hot(kidx.long(), 32).to(dt)
    next_out = onehot * (1 - m) + t["init"].to(dt)[None] * m
    next_idx = torch.where(t["first"][:, None] != 0, t["init_idx"].long()[None], kidx.long())
    out = ol_ref(t, dict(S=c["S"], D=32, act=c["act"]), dt, idx=next_idx)
    out.update(onehot=onehot, next_out=next_out, next_idx=next_idx)
    return out


def sl_floor(c):
    return 0.0 if c["kind"] == "spike" else 1.0


def sl_ratio(c):
    t = sl_inputs(c)
    M, S = c["M"], c["S"]
    q = None if c["smp"] == "mode" else t["q"].reshape(M * S, 32)
    k64, near = draw_ref(t["logit"].reshape(M * S, 32), q, U_MIX)
    assert near.sum().item() <= TIE_CAP * M * S, (c, int(near.sum()))
    a, b = sl_down(t, c, k64.reshape(M, S), F32), sl_down(t, c, k64.reshape(M, S), F64)
    return max(ratio(a[k], b[k], sl_floor(c) if k == "rstd" else 1.0) for k in ("pre", "y", "mean", "rstd", "next_out"))


def sl_call(ops, c, t, o, **over):
    kw = dict(next_first=dev(t["first"]), init=dev(t["init"]), init_idx=dev(t["init_idx"]), next_out=o["next_out"],
              next_idx=o["next_idx"], WT=o["WT"], x2=o["x2"], pre=o["pre"], gamma=dev(t["gamma"]), beta=dev(t["beta"]),
              y=o["y"], mean=o["mean"], rstd=o["rstd"], noise=None if c["smp"] == "mode" else dev(t["q"]),
              idx=o["idx"], forced=None if t["forced"] is None else dev(t["forced"].int()), flips=o["flips"],
              unimix=U_MIX, mode=c["smp"] == "mode", act=c["act"])
    kw.update(over)
    ops.onehot_sample_linear_ln(dev(t["logit"]), o["onehot"], **kw)


def sl_outputs(c, t):
    M, S, N = c["M"], c["S"], c["N"]
    nan = lambda *s: torch.full(s, NAN, device="cuda")
    o = dict(onehot=nan(M, S, 32), next_out=nan(M, S, 32), mean=nan(M), rstd=nan(M),
             next_idx=torch.full((M, S), -1, dtype=torch.int32, device="cuda"),
             idx=torch.full((M, S), -1, dtype=torch.int32, device="cuda") if c["idx"] else None,
             flips=torch.zeros(1, dtype=torch.int32, device="cuda") if c["smp"] == "forced" else None)
    o["pbuf"], o["pre"] = place(torch.full((M, N), NAN), 4, 1, NAN)
    o["ybuf"], o["y"] = place(torch.full((M, N), NAN), 8, 3, NAN)
    o["WT"] = place(t["WT"], 4, 1)[1]
    o["x2"] = place(t["x2"], 3, 2)[1] if t["x2"] is not None else None
    return o


def sl_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@gpu
@pytest.mark.parametrize("c", SL_CASES, ids=sl_id)
def test_onehot_sample_linear_ln(ops, c):
    M, S, N = c["M"], c["S"], c["N"]
    t = sl_inputs(c)
    what = "sample_linear_ln " + sl_id(c)
    q = None if c["smp"] == "mode" else t["q"].reshape(M * S, 32)
    k64, near = draw_ref(t["logit"].reshape(M * S, 32), q, U_MIX)
    k64, near = k64.reshape(M, S), near.reshape(M, S)
    assert near.sum().item() <= TIE_CAP * M * S, f"{what}: {int(near.sum())} near-tie groups"
    o = sl_outputs(c, t)
    sl_call(ops, c, t, o)
    oh = o["onehot"].cpu()
    assert bool(((oh == 0) | (oh == 1)).all()) and bool((oh.sum(-1) == 1).all()), what + ": onehot is not a one-hot"
    kidx = oh.argmax(-1)
    if c["idx"]:
        assert torch.equal(o["idx"].cpu().long(), kidx), what + ": idx is not the class of onehot"
    if c["smp"] == "forced":
        assert torch.equal(kidx, t["forced"]), what + ": the forced class was not taken"
        want = int((k64 != t["forced"]).sum())
        print(f"{what}: flips {int(o['flips'].item())} float64 {want} excluded {int(near.sum())}")
        assert abs(int(o["flips"].item()) - want) <= int(near.sum()), what + ": flips"
    else:
        bad = (kidx != k64) & ~near
        assert not bad.any(), f"{what}: {int(bad.sum())} draws differ from the float64 argmax"
    ref = sl_down(t, c, kidx)
    exact(o["onehot"], ref["onehot"], what + " onehot")
    exact(o["next_out"], ref["next_out"], what + " next_out")
    exact(o["next_idx"], ref["next_idx"], what + " next_idx")
    for buf, off in ((o["pbuf"], 1), (o["ybuf"], 3)):
        assert bool(torch.isnan(buf[:, :off]).all()) and bool(torch.isnan(buf[:, off + N:]).all()), what + ": wrote outside"
    check(o["pre"], ref["pre"], what=what + " pre")
    check(o["y"], ref["y"], what=what + " y")
    check(o["mean"], ref["mean"], what=what + " mean")
    check(o["rstd"], ref["rstd"], what=what + " rstd", floor=sl_floor(c))


@gpu
def test_onehot_sample_linear_ln_rejections(ops):
    """S = 33, N = 1280, N = 255, ldw % 4 != 0 and a runtime activation code through ctypes: DV3_ERR_ARG, nothing
    written.  (The wrapper refuses the same calls before the library sees them.)"""
    M = 3
    g = gen(12)
    logit = dev(torch.randn(M, 33, 32, generator=g))
    q = dev(torch.empty(M, 33, 32).exponential_(generator=g))
    WT = dev(torch.randn(33 * 32, 1284, generator=g))
    first, init, init_idx = dev(torch.zeros(M)), dev(torch.zeros(33, 32)), dev(torch.zeros(33, dtype=torch.int32))
    outs = [torch.full((M * 33 * 32,), NAN, device="cuda") for _ in range(2)] + [torch.full((M, 1284), NAN, device="cuda") for _ in range(2)]
    onehot, next_out, pre, y = outs
    next_idx = torch.full((M * 33,), -1, dtype=torch.int32, device="cuda")
    gm = dev(torch.ones(1284))

    def call(S=7, N=256, ldw=1284, act=1):
        rc = lib().dv3_onehot_sample_linear_ln_fwd(ptr(logit), ptr(q), 0, 0, ptr(onehot), 0, 0, 0, U_MIX, 0, ptr(first),
                                                   ptr(init), ptr(init_idx), ptr(next_out), ptr(next_idx), S, 0, 0, 0,
                                                   ptr(WT), ldw, ptr(pre), 1284, ptr(gm), ptr(gm), ptr(y), 1284, 0, 0, M, N,
                                                   act, stream())
        torch.cuda.synchronize()
        return rc

    for what, kw in (("S = 33", dict(S=33)), ("N = 1280", dict(N=1280)), ("N = 255", dict(N=255)),
                     ("ldw % 4", dict(ldw=1283)), ("act code 5", dict(act=5)), ("act code 2", dict(act=2))):
        assert call(**kw) == ERR_ARG, what
        assert all(bool(torch.isnan(t).all()) for t in outs) and bool((next_idx == -1).all()), what + ": an output was written"
    assert call() == 0


@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_onehot_sample_fwd_blend_entry_point(mode):
    """dv3_onehot_sample_fwd_blend (the ABI form without a wrapper: sample + the next step's reset blend) through
    ctypes against the float64 draw and the blend evaluated on the kernel's own draw; D = 7 and 32."""
    for D, S, M in ((7, 5, 13), (32, 4, 9)):
        g = gen(90 + D + mode)
        R = M * S
        logit, q = cat_logits(R, D, "randn", g), torch.empty(R, D).exponential_(generator=g)
        first = (torch.arange(M) % 3 == 1).float()
        init = F.one_hot(torch.randint(0, D, (S,), generator=g), D).float()
        k64, near = draw_ref(logit, None if mode else q, U_MIX)
        assert near.sum().item() <= TIE_CAP * R
        onehot, next_out = torch.full((R, D), NAN, device="cuda"), torch.full((R, D), NAN, device="cuda")
        ld, qd, fd, idv = dev(logit), dev(q), dev(first), dev(init)
        rc = lib().dv3_onehot_sample_fwd_blend(ptr(ld), ptr(qd), 0, 0, ptr(onehot), R, D, U_MIX, mode, ptr(fd), ptr(idv),
                                               ptr(next_out), S, stream())
        torch.cuda.synchronize()
        assert rc == 0
        oh = onehot.cpu()
        kidx = oh.argmax(-1)
        what = f"onehot_sample_fwd_blend D={D} mode={mode}"
        exact(oh, F.one_hot(kidx, D), what + " onehot")
        assert not ((kidx != k64) & ~near).any(), what + ": draws differ from the float64 argmax"
        m = first.double()[:, None, None]
        exact(next_out, (oh.double().reshape(M, S, D) * (1 - m) + init.double()[None] * m).reshape(R, D), what + " next_out")


# ====================================================================================================== C. actor_head
AH_U = [1, 63, 64, 65, 256, 257, 512, 513, 1024]
AH_A = [1, 5, 6, 7, 12, 13, 32, 33, 64]
STD_RANGES = [(0.1, 1.0), (0.05, 2.0)]


def AH(M, U, A, onehot, std=0, unimix=0.01, act=True, sat=False, tie=False, kind="randn"):
    return dict(M=M, U=U, A=A, onehot=onehot, std=std, unimix=unimix, act=act, sat=sat, tie=tie, kind=kind)


def ah_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


AH_GRID = {U: [AH(49, U, A, oh, std=(U + A) % 2) for A in AH_A for oh in (False, True)] for U in AH_U}
AH_EXTRA = ([AH(1, 300, 7, oh) for oh in (False, True)] + [AH(16384 + 5, 16, 3, oh) for oh in (False, True)] +
            [AH(49, 100, 6, False, sat=True, std=s) for s in (0, 1)] +
            [AH(49, 100, 6, True, unimix=0.0), AH(49, 100, 1, True, unimix=0.0), AH(49, 100, 5, True, tie=True),
             AH(49, 300, 6, False, act=False), AH(49, 600, 6, True, act=RT_ACT), AH(49, 40, 6, False, act=RT_ACT)] +
            [AH(5, U, 6, oh, kind=k) for U, oh in ((33, False), (132, True)) for k in LN_KINDS[1:]])
AH_CASES = [c for cs in AH_GRID.values() for c in cs] + AH_EXTRA


def ah_inputs(c):
    M, U, A = c["M"], c["U"], c["A"]
    g = gen(seed_of(c, 5))
    pre = rows_of(M, U, c["kind"], g)
    gamma, beta = 1 + 0.1 * torch.randn(U, generator=g), 0.1 * torch.randn(U, generator=g)
    Wm, bm = torch.randn(A, U, generator=g) / math.sqrt(U), 0.1 * torch.randn(A, generator=g)
    Ws, bs = torch.randn(A, U, generator=g) / math.sqrt(U), 0.1 * torch.randn(A, generator=g)
    if c["sat"]:  # std raw +-30, mean raw +-10
        bs[0], bs[1], bm[2], bm[3] = 30.0, -30.0, 10.0, -10.0
    noise = torch.empty(M, A).exponential_(generator=g) if c["onehot"] else torch.randn(M, A, generator=g)
    if c["tie"]:  # classes 1 and A - 1 are the same head with the same noise, and the likeliest
        Wm[A - 1], bm[1], bm[A - 1] = Wm[1], 6.0, 6.0
        noise[:, A - 1] = noise[:, 1]
    forced = torch.randint(0, A, (M,), generator=g)
    return dict(pre=pre, gamma=gamma, beta=beta, Wm=Wm, bm=bm, Ws=Ws, bs=bs, noise=noise, forced=forced)


def ah_ref(t, c, dt=F64, noise=None, kidx=None):
    """-> dict(y, mean, rstd, out_m, [out_s,] action, ent [, idx, near]).  kidx: evaluate the action on that draw."""
    y, mean, rstd = ln_act(t["pre"].to(dt), t["gamma"].to(dt), t["beta"].to(dt), c["act"])
    head = lambda W, b: (y[:, None, :] * t[W].to(dt)[None]).sum(-1) + t[b].to(dt)  # (one order for every output)
    om = head("Wm", "bm")
    out = dict(y=y, mean=mean, rstd=rstd, out_m=om)
    nz = (t["noise"] if noise is None else noise).to(dt)
    if not c["onehot"]:
        lo, hi = STD_RANGES[c["std"]]
        osd = head("Ws", "bs")
        mu, sd = torch.tanh(om), (hi - lo) * torch.sigmoid(osd + 2.0) + lo
        a = mu + sd * nz
        out.update(out_s=osd, action=a / a.abs().clamp_min(1.0), raw=a,
                   ent=(0.5 + 0.5 * math.log(2 * math.pi) + torch.log(sd)).sum(-1))
        return out
    A = c["A"]
    p = F.softmax(om, -1) * (1 - c["unimix"]) + c["unimix"] / A
    idx, near = draw_ref(om, nz, c["unimix"], dt)
    k = idx if kidx is None else kidx.long()
    out.update(action=F.one_hot(k, A).to(dt), ent=-(p * torch.log(p)).sum(-1), idx=idx, near=near)
    return out


AH_KEYS = ("y", "mean", "rstd", "out_m", "out_s", "action", "ent")


def ah_floor(c):
    return 0.0 if c["kind"] == "spike" else 1.0


def ah_ratio(c):
    t = ah_inputs(c)
    a, b = ah_ref(t, c, F32), ah_ref(t, c, F64)
    if c["onehot"]:
        n_ex = int((b["near"]).sum())
        assert n_ex <= TIE_CAP * c["M"], (c, n_ex)
        a = ah_ref(t, c, F32, kidx=b["idx"])
    return max(ratio(a[k], b[k], ah_floor(c) if k == "rstd" else 1.0) for k in AH_KEYS if k in b)


def run_ah(ops, c, *, forced=False, philox=False, stats=True, alias_eps=False, act_idx=True):
    M, U, A, oh = c["M"], c["U"], c["A"], c["onehot"]
    t = ah_inputs(c)
    what = f"actor_head {ah_id(c)}" + (" forced" if forced else "") + (" philox" if philox else "")
    nan = lambda *s: torch.full(s, NAN, device="cuda")
    pre = place(t["pre"], 6 - (U + 1) % 2, 2)[1]  # an odd leading dimension
    ybuf, y = place(torch.full((M, U), NAN), 8 - (U + 1) % 2, 3, NAN)
    assert pre.stride(0) % 2 == 1 and y.stride(0) % 2 == 1 or M == 1
    mean, rstd = (nan(M), nan(M)) if stats else (None, None)
    out_m, out_s, action, ent = nan(M, A), None if oh else nan(M, A), nan(M, A), nan(M)
    noise = None if philox else dev(t["noise"])
    eps_out = None if oh else (noise if alias_eps else nan(M, A))
    kidx_d = torch.full((M,), -1, dtype=torch.int32, device="cuda") if oh and act_idx else None
    flips = torch.zeros(1, dtype=torch.int32, device="cuda") if forced else None
    lo, hi = STD_RANGES[c["std"]]
    ops.actor_head(pre, dev(t["gamma"]), dev(t["beta"]), y, mean, rstd, dev(t["Wm"]), dev(t["bm"]),
                   None if oh else dev(t["Ws"]), None if oh else dev(t["bs"]), out_m, out_s, action, ent, noise=noise,
                   rng=ops.RngStream("cuda", seed=77) if philox else None, eps_out=eps_out, act_idx=kidx_d,
                   forced=dev(t["forced"].int()) if forced else None, flips=flips, min_std=lo, max_std=hi,
                   unimix=c["unimix"], onehot=oh, act=c["act"])
    assert bool(torch.isnan(ybuf[:, :3]).all()) and bool(torch.isnan(ybuf[:, 3 + U:]).all()), what + ": wrote outside y"
    used = None
    if not oh:
        used = eps_out.cpu()
        if philox:
            assert bool(torch.isfinite(used).all()) and used.abs().max().item() < 8, what + ": eps_out"
        else:
            exact(used, t["noise"], what + " eps_out")
    ref = ah_ref(t, c, noise=used)
    kidx = None
    if oh:
        ac = action.cpu()
        assert bool(((ac == 0) | (ac == 1)).all()) and bool((ac.sum(-1) == 1).all()), what + ": action is not a one-hot"
        kidx = ac.argmax(-1)
        if kidx_d is not None:
            assert torch.equal(kidx_d.cpu().long(), kidx), what + ": act_idx is not the class of action"
        n_ex = int(ref["near"].sum())
        assert n_ex <= TIE_CAP * M, f"{what}: {n_ex} near-tie rows"
        if forced:
            assert torch.equal(kidx, t["forced"]), what + ": the forced class was not taken"
            want = int((ref["idx"] != t["forced"]).sum())
            print(f"{what}: flips {int(flips.item())} float64 {want} excluded {n_ex}")
            assert abs(int(flips.item()) - want) <= n_ex, what + ": flips"
        else:
            bad = (kidx != ref["idx"]) & ~ref["near"]
            assert not bad.any(), f"{what}: {int(bad.sum())} draws differ from the float64 argmax"
            if c["tie"]:
                assert int((ref["idx"] == 1).sum()) > M // 2 and not bool((kidx == A - 1).any()), what + ": tie"
        ref = ah_ref(t, c, kidx=kidx)
    elif not philox and M >= 48 and A >= 5:
        assert bool((ref["raw"].abs() > 1).any()) and bool((ref["raw"].abs() < 1).any())  # both sides of the rescale
    got = dict(y=y, mean=mean, rstd=rstd, out_m=out_m, out_s=out_s, action=action, ent=ent)
    for k in AH_KEYS:
        if got[k] is not None:
            check(got[k], ref[k], what=f"{what} {k}", floor=ah_floor(c) if k == "rstd" else 1.0)


@gpu
@pytest.mark.parametrize("U", AH_U)
def test_actor_head_every_width(ops, U):
    """Every A of AH_A (a full batch, a remainder and a second batch of OB = 12 / 6 outputs) at this U, both actors,
    M = 49 rows (every rotation of the batch)."""
    for c in AH_GRID[U]:
        run_ah(ops, c)


@gpu
@pytest.mark.parametrize("c", AH_EXTRA, ids=ah_id)
def test_actor_head_forms(ops, c):
    run_ah(ops, c)


@gpu
@pytest.mark.parametrize("oh", [False, True])
def test_actor_head_call_forms(ops, oh):
    """mean / rstd None, eps_out aliasing noise, act_idx None, forced + flips, and the Philox path (eps_out is taken as
    given: the action must be the float64 one computed from it)."""
    c = AH(49, 257, 7, oh)
    run_ah(ops, c, stats=False, alias_eps=not oh, act_idx=False)
    if oh:
        run_ah(ops, c, forced=True)
        run_ah(ops, AH(16384 + 5, 16, 3, True), forced=True)
    else:
        run_ah(ops, c, philox=True)


@gpu
def test_actor_head_rejections(ops):
    """U = 1025 and A = 65 through ctypes (the wrapper refuses them too): DV3_ERR_ARG, outputs still NaN."""
    M = 3
    pre, W = dev(torch.randn(M, 1025)), dev(torch.randn(65, 1025))
    v = dev(torch.ones(1025))
    outs = [torch.full((M, 1025), NAN, device="cuda") for _ in range(5)]
    y, out_m, out_s, action, eps = outs

    def call(U, A, act=1):
        rc = lib().dv3_actor_head_fwd_ex(ptr(pre), 1025, ptr(v), ptr(v), ptr(y), 1025, 0, 0, ptr(W), ptr(v), ptr(W), ptr(v),
                                         ptr(out_m), ptr(out_s), ptr(pre), 0, 0, ptr(eps), ptr(action), 0, 0, 0, 0, M, U, A,
                                         0.1, 1.0, 0.01, 0, act, stream())
        torch.cuda.synchronize()
        return rc

    for U, A, act in ((1025, 6, 1), (64, 65, 1), (64, 6, 9)):
        assert call(U, A, act) == ERR_ARG, (U, A, act)
        assert all(bool(torch.isnan(t).all()) for t in outs), (U, A, act, "an output was written")
    assert call(1024, 64) == 0


# =========================================================================== D. transpose2d(_many), onehot_to_idx
TR_SIZES = [1, 31, 32, 33, 65]


@gpu
@pytest.mark.parametrize("R", TR_SIZES)
def test_transpose2d(ops, R):
    for C in TR_SIZES:
        src = torch.randn(R, C, generator=gen(R * 100 + C))
        sbuf, s = place(src, 5, 2)
        dbuf, d = place(torch.full((C, R), NAN), 3, 1, NAN)
        ops.transpose2d(s, d)
        exact(d, src.t(), f"transpose2d {R}x{C}")
        assert outside_untouched(dbuf, 1, R, NAN), f"transpose2d {R}x{C}: wrote outside dst"


TR_JOBS = [(65, 33), (1, 1), (130, 7), (32, 32), (1, 70), (31, 1), (33, 65), (64, 64), (5, 5), (1, 1), (100, 3), (2, 97), (40, 41)]


@gpu
@pytest.mark.parametrize("n", [1, 12, 13])
def test_transpose2d_many(ops, n):
    """1, 12 and 13 (two launches) jobs of different sizes, a 1 x 1 job between large ones."""
    g = gen(40 + n)
    srcs = [torch.randn(R, C, generator=g) for R, C in TR_JOBS[:n]]
    pairs, bufs = [], []
    for s in srcs:
        R, C = s.shape
        dbuf, d = place(torch.full((C, R), NAN), 3, 1, NAN)
        pairs.append((place(s, 5, 2)[1], d))
        bufs.append(dbuf)
    ops.transpose2d_many(pairs)
    for k, (s, (_, d)) in enumerate(zip(srcs, pairs)):
        exact(d, s.t(), f"transpose2d_many job {k} of {n} {tuple(s.shape)}")
        assert outside_untouched(bufs[k], 1, s.shape[0], NAN), f"job {k}: wrote outside dst"


@gpu
def test_transpose2d_many_rejects_13_jobs():
    import numpy as np

    srcs = [dev(torch.randn(4, 5)) for _ in range(13)]
    dsts = [torch.full((5, 4), NAN, device="cuda") for _ in range(13)]
    jobs = np.array([(s.data_ptr(), d.data_ptr(), 5, 4, 4, 5) for s, d in zip(srcs, dsts)], dtype=np.uint64)
    assert lib().dv3_transpose2d_many(13, jobs.ctypes.data, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(d).all()) for d in dsts)
    assert lib().dv3_transpose2d_many(12, jobs.ctypes.data, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dsts[12]).all()) and torch.equal(dsts[11].cpu(), srcs[11].cpu().t())


O2I_D = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]


def o2i_group(D):
    G = 4
    while G < 64 and G < D:
        G <<= 1
    return G


@gpu
@pytest.mark.parametrize("D", O2I_D)
def test_onehot_to_idx(ops, D):
    """R = 77 and one row count past the 8192-workgroup cap of this D's group width; group 0 all zero (-> 0), group 1
    not a one-hot with two equal maxima (-> the first), group 2 a plain vector of values."""
    for R in (77, 8192 * (256 // o2i_group(D)) + 3):
        g = gen(D * 7 + R % 5)
        x = F.one_hot(torch.randint(0, D, (R,), generator=g), D).float()
        x[0] = 0.0
        x[1] = 0.25
        x[1, D // 2] = x[1, D - 1] = 2.0
        x[2] = torch.randn(D, generator=g)
        idx = torch.full((R,), -1, dtype=torch.int32, device="cuda")
        ops.onehot_to_idx(dev(x), idx)
        exact(idx, x.double().argmax(-1), f"onehot_to_idx D={D} R={R}")
        assert int(idx[0]) == 0 and int(idx[1]) == D // 2


@gpu
def test_onehot_to_idx_rejects_65_classes():
    x, idx = dev(torch.ones(4, 65)), torch.full((4,), -1, dtype=torch.int32, device="cuda")
    assert lib().dv3_onehot_to_idx(ptr(x), ptr(idx), 4, 65, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((idx == -1).all())


# ===================================================================================================== E. gemm_sample
def GS(M, N, K, bias=True, smp="noise", idx=True, ln=None, kind="randn", K1=0, lay="plain", key=None):
    """ln: None | "stats" | "nostats" (LayerNorm + SiLU of A on load).  K1 > 0: [A | A2] with the seam at K1 (ctypes).
    lay: "plain" | "win4" (A a column window, lda % 4 == 0, 16-byte aligned) | "off1" (A 4-byte aligned: no l16).
    key: the profile key the call must report (l16+sample / direct32x64+sample)."""
    return dict(M=M, N=N, K=K, bias=bias, smp=smp, idx=idx, ln=ln, kind=kind, K1=K1, lay=lay, key=key)


DIRECT, L16S = "gemm_kernel<direct32x64+sample,tA=0,tB=1>", "gemm_kernel<l16+sample,tA=0,tB=1>"
# 129 tiles of 64 x 64 is the smallest output pick_tile sends to the k-contiguous LDS tiles (t64 > 128): M <= 64, N = 8256
GS_CASES = ([GS(33, 128, K, key=DIRECT) for K in (3, 15, 16, 17, 49, 497, 512)] +
            [GS(33, 8256, 32, key=L16S), GS(33, 8256, 48, key=DIRECT), GS(33, 8256, 32, lay="off1", key=DIRECT)] +
            [GS(M, N, 40, bias=(M + N // 64) % 2 == 0) for M in (1, 31, 33, 100) for N in (64, 128, 192)] +
            [GS(33, 128, 40, smp="mode"), GS(33, 128, 40, smp="forced"), GS(33, 128, 40, idx=False)] +
            [GS(33, 128, K, ln="stats", lay="win4") for K in (4, 36, 512)] + [GS(33, 128, 36, ln="nostats")] +
            [GS(5, 64, 36, ln="stats", kind=k) for k in LN_KINDS[1:]] +
            [GS(33, 128, 56, K1=k1) for k1 in (16, 32, 48)])


def gs_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k != "key")


def gs_inputs(c, mode):
    M, N, K, K1 = c["M"], c["N"], c["K"], c["K1"]
    g = gen(seed_of(c, 977 if mode == "int" else 2))
    draw = (lambda *s: ints(s, g)) if mode == "int" else (lambda *s: torch.randn(*s, generator=g))
    X = rows_of(M, K, c["kind"], g) if c["ln"] else draw(M, K)
    B = draw(N, K) if mode == "int" else 2 * torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = draw(N) if c["bias"] else None
    q = torch.empty(M, N).exponential_(generator=g)
    forced = torch.randint(0, 32, (M * N // 32,), generator=g) if c["smp"] == "forced" else None
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    return dict(A=X[:, :K1] if K1 else X, A2=X[:, K1:] if K1 else None, B=B, bias=bias, q=q, forced=forced, gamma=gamma,
                beta=beta)


def gs_ref(t, c, dt=F64):
    """-> dict(logit [, mean, rstd]): [A | A2] B^T + bias, A through LayerNorm + SiLU first when ln is set."""
    X = t["A"].to(dt)
    out = {}
    if c["ln"]:
        X, out["mean"], out["rstd"] = ln_act(X, t["gamma"].to(dt), t["beta"].to(dt), True)
    if t["A2"] is not None:
        X = torch.cat([X, t["A2"].to(dt)], 1)
    out["logit"] = X @ t["B"].to(dt).t() + (t["bias"].to(dt) if t["bias"] is not None else 0.0)
    return out


def gs_draw(t, c, logit):
    M, N = c["M"], c["N"]
    return draw_ref(logit.reshape(M * N // 32, 32), None if c["smp"] == "mode" else t["q"].reshape(M * N // 32, 32), U_MIX)


def gs_ratio(c):
    t = gs_inputs(c, "randn")
    a, b = gs_ref(t, c, F32), gs_ref(t, c, F64)
    _, near = gs_draw(t, c, b["logit"])
    assert near.sum().item() <= TIE_CAP * near.numel(), (c, int(near.sum()))
    return max(ratio(a[k], b[k], 0.0 if k == "rstd" and c["kind"] == "spike" else 1.0) for k in b)


def gs_place(x, lay):
    if x is None or lay == "plain":
        return None if x is None else dev(x)
    if lay == "win4":
        return place(x, 8, 4)[1]
    buf = torch.full((x.numel() + 8,), PAD, device="cuda")
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def run_gs(ops, c, mode):
    M, N, K, K1 = c["M"], c["N"], c["K"], c["K1"]
    t = gs_inputs(c, mode)
    ref = gs_ref(t, c)
    what = f"gemm_sample {gs_id(c)} {mode}"
    R = M * N // 32
    A, A2, B = gs_place(t["A"], c["lay"]), gs_place(t["A2"], "plain"), dev(t["B"])
    cbuf, C = place(torch.full((M, N), NAN), 4, 0, NAN)
    onehot = torch.full((M, N), NAN, device="cuda")
    idx = torch.full((R,), -1, dtype=torch.int32, device="cuda") if c["idx"] else None
    flips = torch.zeros(1, dtype=torch.int32, device="cuda") if c["smp"] == "forced" else None
    forced = dev(t["forced"].int()) if c["smp"] == "forced" else None
    bias = dev(t["bias"]) if c["bias"] else None
    noise = None if c["smp"] == "mode" else dev(t["q"])
    mean, rstd = ((torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")) if c["ln"] == "stats"
                  else (None, None))
    if K1:
        rc = lib().dv3_gemm_sample_f32(M, N, K, ptr(A), A.stride(0), ptr(A2), A2.stride(0), K1, ptr(B), K, ptr(C),
                                       C.stride(0), ptr(bias), ptr(noise), 0, 0, ptr(onehot), ptr(idx), ptr(forced),
                                       ptr(flips), U_MIX, int(c["smp"] == "mode"), 0, 0, 0, 0, stream())
        assert rc == 0, what
    else:
        ops.PROFILE.start()
        ops.PROFILE.by_shape = False
        ops.gemm_sample(A, B, C, onehot, bias=bias, noise=noise, idx=idx, forced=forced, flips=flips, unimix=U_MIX,
                        mode=c["smp"] == "mode", ln=(dev(t["gamma"]), dev(t["beta"]), mean, rstd) if c["ln"] else None)
        keys = list(ops.PROFILE.stop())
        if c["key"]:
            assert keys == [c["key"]], (what, keys)
    assert bool(torch.isnan(cbuf[:, N:]).all()), what + ": wrote outside the logits"
    oh = onehot.cpu()
    assert bool(((oh == 0) | (oh == 1)).all()) and bool((oh.reshape(R, 32).sum(-1) == 1).all()), what + ": onehot"
    kidx = oh.reshape(R, 32).argmax(-1)
    if c["idx"]:
        assert torch.equal(idx.cpu().long(), kidx), what + ": idx is not the class of onehot"
    if mode == "int":
        assert 3 + 9 * K < 2 ** 23  # every partial sum is an integer fp32 holds
        return exact(C, ref["logit"], what + " logit")
    check(C, ref["logit"], what=what + " logit")
    if c["ln"] == "stats":
        check(mean, ref["mean"], what=what + " ln mean")
        check(rstd, ref["rstd"], what=what + " ln rstd", floor=0.0 if c["kind"] == "spike" else 1.0)
    k64, near = gs_draw(t, c, ref["logit"])
    assert near.sum().item() <= TIE_CAP * R, f"{what}: {int(near.sum())} near-tie groups"
    if c["smp"] == "forced":
        assert torch.equal(kidx, t["forced"]), what + ": the forced class was not taken"
        want = int((k64 != t["forced"]).sum())
        print(f"{what}: flips {int(flips.item())} float64 {want} excluded {int(near.sum())}")
        assert abs(int(flips.item()) - want) <= int(near.sum()), what + ": flips"
    else:
        bad = (kidx != k64) & ~near
        assert not bad.any(), f"{what}: {int(bad.sum())} draws differ from the float64 argmax"


@gpu
@pytest.mark.parametrize("c", GS_CASES, ids=gs_id)
def test_gemm_sample(ops, c):
    run_gs(ops, c, "randn")
    if not c["ln"]:
        run_gs(ops, c, "int")


@gpu
def test_gemm_sample_rejections():
    """A seam off the 16-k chunk boundary, LayerNorm on load together with A2, N % 64 != 0: DV3_ERR_ARG, nothing written."""
    M, N, K = 33, 128, 56
    g = gen(13)
    A, A2, B = dev(torch.randn(M, K, generator=g)), dev(torch.randn(M, K, generator=g)), dev(torch.randn(N, K, generator=g))
    q, v = dev(torch.empty(M, N).exponential_(generator=g)), dev(torch.ones(K))
    C, onehot = torch.full((M, N), NAN, device="cuda"), torch.full((M, N), NAN, device="cuda")

    def call(N=N, K1=16, a2=A2, gamma=None):
        rc = lib().dv3_gemm_sample_f32(M, N, K, ptr(A), K, ptr(a2), K, K1, ptr(B), K, ptr(C), N, 0, ptr(q), 0, 0, ptr(onehot),
                                       0, 0, 0, U_MIX, 0, ptr(gamma), ptr(gamma), 0, 0, stream())
        torch.cuda.synchronize()
        return rc

    for what, kw in (("K1 = 8", dict(K1=8)), ("K1 = 24", dict(K1=24)), ("K1 = K", dict(K1=K)), ("ln with A2", dict(gamma=v)),
                     ("N = 96", dict(N=96, a2=None))):
        assert call(**kw) == ERR_ARG, what
        assert bool(torch.isnan(C).all()) and bool(torch.isnan(onehot).all()), what + ": an output was written"


# ============================================================= G. colsum, colsum_grouped, tensorstats, quantile2_ema
# (R, N, columns of padding): the slab kernel (one slab: no atomics; 65 rows: the first atomic slabs; 64 * 64 + 1: the
# slab cap), the narrow kernel from R = 4096 at N <= 32 (N = 7, 31: the rounding of its block count), one case past
# its 1024-workgroup cap
CS_CASES = [(1, 33, 0), (64, 64, 0), (65, 65, 3), (64 * 64 + 1, 200, 0), (4095, 32, 0), (4096, 33, 0), (4096, 32, 0),
            (4096, 32, 5), (4096, 7, 0), (5000, 31, 2), (4096, 1, 0), (1024 * 256 * 64 // 32 + 64, 32, 0)]


def cs_inputs(R, N, kind):
    g = gen(R * 131 + N + (977 if kind == "int" else 0))
    x = ints((R, N), g) if kind == "int" else torch.randn(R, N, generator=g)
    out0 = ints((N,), g) if kind == "int" else torch.randn(N, generator=g)
    return x, out0


def cs_ref(x, out0, acc, dt=F64):
    s = x.to(dt).sum(0)
    return s + out0.to(dt) if acc else s


@gpu
@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("R,N,pad", CS_CASES)
def test_colsum(ops, R, N, pad, kind):
    x, out0 = cs_inputs(R, N, kind)
    xd = place(x, pad, pad // 2)[1]
    assert 3 * (R + 1) < 2 ** 23
    for acc in (False, True):
        out = dev(out0.clone()) if acc else torch.full((N,), NAN, device="cuda")
        ops.colsum(xd, out, accumulate=acc)
        what = f"colsum {R}x{N} ld {N + pad} acc={acc} {kind}"
        if kind == "int":
            exact(out, cs_ref(x, out0, acc), what)
        else:
            check(out, cs_ref(x, out0, acc), what=what)


CG_R, CG_N = [1, 64, 65, 4097], [1, 64, 65]


def cg_items(n, kind):
    g = gen(70 + n + (977 if kind == "int" else 0))
    draw = (lambda *s: ints(s, g)) if kind == "int" else (lambda *s: torch.randn(*s, generator=g))
    return [(draw(CG_R[k % 4], CG_N[(k // 4) % 3]), draw(CG_N[(k // 4) % 3])) for k in range(n)]


def cg_call(xs, outs):
    import ctypes

    n = len(xs)
    col = lambda vals, ty: (ty * n)(*vals)
    rc = lib().dv3_colsum_grouped(n, col([x.data_ptr() for x in xs], ctypes.c_void_p), col([x.stride(0) for x in xs], ctypes.c_long),
                                  col([o.data_ptr() for o in outs], ctypes.c_void_p), col([x.shape[0] for x in xs], ctypes.c_long),
                                  col([x.shape[1] for x in xs], ctypes.c_int), stream())
    torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("n", [1, 48])
def test_colsum_grouped(n, kind):
    """out_k += column sums of x_k for 1 and 48 items of mixed sizes (row-strided x), prefilled outputs."""
    items = cg_items(n, kind)
    xs = [place(x, 3, 1)[1] for x, _ in items]
    outs = [dev(o.clone()) for _, o in items]
    assert cg_call(xs, outs) == 0
    for k, (x, o) in enumerate(items):
        what = f"colsum_grouped item {k} of {n} {tuple(x.shape)} {kind}"
        if kind == "int":
            exact(outs[k], cs_ref(x, o, True), what)
        else:
            check(outs[k], cs_ref(x, o, True), what=what)


@gpu
def test_colsum_grouped_rejects_49_items():
    items = cg_items(48, "int")
    items.append(items[0])
    xs, outs = [dev(x) for x, _ in items], [dev(o.clone()) for _, o in items]
    assert cg_call(xs, outs) == ERR_ARG
    assert all(torch.equal(o.cpu(), o0) for o, (_, o0) in zip(outs, items)), "an output was written"


TS_N = [1, 3, 4, 5, 1023, 1025]


def ts_data(n, kind, g):
    if kind == "const":
        return torch.full((n,), 0.75)
    z = torch.randn(n, generator=g)
    return z * 3 + 1.5 if kind == "randn" else z + 1e4


def ts_ref(x, dt=F64):
    x = x.to(dt)
    return torch.stack([x.mean(), x.std() if x.numel() > 1 else x.mean() * float("nan"), x.min(), x.max()])


TS_CASES = [(n, "randn", off) for n in TS_N for off in (0, 1)] + [(1025, "const", 0), (1025, "offset", 0), (1025, "offset", 1)]
TS_NAMES = ("mean", "std", "min", "max")


def ts_check(got, ref, what):
    got, ref = got.cpu(), ref.cpu()
    for k, nm in enumerate(TS_NAMES):
        if ref[k] != ref[k]:
            assert got[k] != got[k], f"{what} {nm}: expected NaN (one element has no unbiased std)"
        else:
            check(got[k:k + 1], ref[k:k + 1], what=f"{what} {nm}")


@gpu
@pytest.mark.parametrize("n,kind,off", TS_CASES)
def test_tensorstats(ops, n, kind, off):
    """off = 1: x[1:] of a buffer, a 4-byte-aligned base (the scalar path)."""
    x = ts_data(n, kind, gen(n * 3 + off))
    xd = dev(torch.cat([torch.full((off,), 1e9), x]))[off:]
    assert xd.data_ptr() % 16 == 4 * off and xd.is_contiguous()
    out = torch.full((4,), 7.0, device="cuda")
    ops.tensorstats(xd, out)
    ts_check(out, ts_ref(x), f"tensorstats n={n} {kind} off={off}")


@gpu
@pytest.mark.parametrize("count", [1, 6])
def test_tensorstats_multi(ops, count):
    g = gen(80 + count)
    xs = [ts_data(n, "randn", g) * (i + 1) for i, n in enumerate((1025, 5, 1, 1023, 4, 3)[:count])]
    out = torch.full((count, 4), 7.0, device="cuda")
    ops.tensorstats_multi([(dev(x), None, None) for x in xs], out)
    for i, x in enumerate(xs):
        ts_check(out[i], ts_ref(x), f"tensorstats_multi job {i} of {count} n={x.numel()}")


Q_N = [8192, 8193, 16384, 16385]  # 16 values per thread stay in registers up to 16384; 8 per trip of the streamed loop
Q_KINDS = ["randn", "inf", "equal", "negative", "denormal"]
Q_QS = [(0.05, 0.95), (0.0, 1.0), (0.5, 0.5)]


def q_data(n, kind, g):
    x = torch.randn(n, generator=g) * 3 + 0.5
    if kind == "inf":
        x[n // 3], x[n // 2] = float("inf"), float("-inf")
    elif kind == "equal":
        x = torch.full((n,), 0.3)
    elif kind == "negative":
        x = -x.abs() - 1.0
    elif kind == "denormal":
        x = x * 1e-41
    return x


def q_pairs(kind):
    return Q_QS[:1] if kind == "inf" else Q_QS  # (q = 0 / 1 would interpolate between infinities)


@gpu
@pytest.mark.parametrize("kind", Q_KINDS)
@pytest.mark.parametrize("n", Q_N)
def test_quantile2_ema(ops, n, kind):
    """As tests/test_kernels_gpu.py::test_quantile_ema_matches_torch_quantile: the fp32 result equals torch.quantile's
    to the last ulp of the interpolation and the float64 quantile to 1e-6; alpha = 0 leaves the EMA, alpha = 1 replaces it."""
    x = q_data(n, kind, gen(n + Q_KINDS.index(kind)))
    xd = dev(x)
    for q0, q1 in q_pairs(kind):
        ref32 = torch.quantile(x, torch.tensor([q0, q1]))
        ref64 = torch.quantile(x.double(), torch.tensor([q0, q1], dtype=F64))
        out = torch.full((2,), NAN, device="cuda")
        ops.quantile2_ema(xd, q0, q1, out_q=out)
        what = f"quantile2_ema n={n} {kind} q=({q0}, {q1})"
        err = (out.cpu() - ref32).abs()
        print(f"{what}: max err {err.max().item():.3e} bar {1.2e-7 * max(1.0, ref32.abs().max().item()):.3e}")
        assert bool((err <= 1.2e-7 * ref32.abs().clamp_min(1.0)).all()), (what, out.cpu(), ref32)
        check(out, ref64, tol=1e-6, what=what + " f64")
        for alpha in (0.0, 1.0):
            ema = torch.tensor([0.3, 2.0], device="cuda")
            ops.quantile2_ema(xd, q0, q1, ema=ema, alpha=alpha)
            assert torch.equal(ema.cpu(), out.cpu() if alpha else torch.tensor([0.3, 2.0])), (what, alpha)


# ============================================================================================ the oracle's own error
def g_ratio():
    worst = 0.0
    for R, N, _ in CS_CASES:
        x, out0 = cs_inputs(R, N, "randn")
        worst = max(worst, ratio(cs_ref(x, out0, True, F32), cs_ref(x, out0, True)))
    for x, o in cg_items(48, "randn"):
        worst = max(worst, ratio(cs_ref(x, o, True, F32), cs_ref(x, o, True)))
    for n, kind, off in TS_CASES:
        x = ts_data(n, kind, gen(n * 3 + off))
        a, b = ts_ref(x, F32), ts_ref(x)
        worst = max([worst] + [ratio(a[k:k + 1], b[k:k + 1]) for k in range(4) if b[k] == b[k]])
    return worst


def group_ratios():
    return {"A": max(ol_ratio(c) for c in OL_CASES), "B": max(sl_ratio(c) for c in SL_CASES),
            "C": max(ah_ratio(c) for c in AH_CASES), "E": max(gs_ratio(c) for c in GS_CASES), "G": g_ratio()}


def test_fp32_oracle_error_is_under_half_the_bar():
    """No bar is widened: on every case of groups A, B, C, E, G the same reference evaluated in fp32 on the CPU stays under
    half of the bar from the float64 one, and the float64 draws alone meet the near-tie cap.  CPU only; no kernel."""
    worst = group_ratios()
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v < 0.5 for v in worst.values()), worst
