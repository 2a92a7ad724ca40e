"""Segment-sum weight gradient over one-hot inputs (ops.onehot_wgrad, csrc/onehot_wgrad.hip) against a float64
segment sum built on the host from the class indices, and the engines that use it against their dense launches.

Every output element is held to the bound any-order float32 summation guarantees (Higham, Accuracy and Stability of
Numerical Algorithms, 4.2):  |err| <= gamma_n * (|gW0| + sum |dY terms|),  gamma_n = n u / (1 - n u),  u = 2^-24,
with n = rows in the segment + number of row splits + 1 (the adds inside the splits, the adds of the partials, the
add into gW).  No tuned tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U24 / (1.0 - n * U24)


def _reference(dY, idx, D, gW0):
    """float64 segment sum -> (ref, sum of absolute terms, rows per segment), each [U, S*D] / [S*D]."""
    dY64 = dY.detach().cpu().double().numpy()
    ix = idx.detach().cpu().numpy()
    g0 = gW0.detach().cpu().double().numpy()
    R, S = ix.shape
    oh = np.zeros((R, S * D))
    oh[np.arange(R)[:, None], np.arange(S)[None, :] * D + ix] = 1.0
    return g0 + dY64.T @ oh, np.abs(g0) + np.abs(dY64).T @ oh, oh.sum(0)


def _check(got, dY, idx, D, gW0, nsplit):
    ref, mag, rows = _reference(dY, idx, D, gW0)
    err = np.abs(got.detach().cpu().double().numpy() - ref)
    bound = _gamma(rows + nsplit + 1)[None, :] * mag
    worst = float((err - bound).max())
    print(f"max err {err.max():.3e}  max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert worst <= 0.0, f"error exceeds the summation bound by {worst:.3e}"


def _inputs(R, U, S, D, seed=0, dev="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dY = torch.randn(R, U, generator=g).to(dev)
    idx = torch.randint(0, D, (R, S), generator=g, dtype=torch.int32).to(dev)
    return dY, idx


def _run(dY, idx, D, gW, nsplit=None):
    from dv3hip import ops

    R, S = idx.shape
    U = dY.shape[1]
    part = torch.empty(max(ops.onehot_wgrad_partials(R, U, S, D), (nsplit or 1) * -(-U // 32) * S * D * 32),
                       device=dY.device)
    ops.onehot_wgrad(dY, idx, D, gW, part, nsplit=nsplit)
    torch.cuda.synchronize()
    return gW


def _splits(R, U, nsplit=None):
    from dv3hip import ops

    if nsplit is None:
        nsplit = ops.onehot_wgrad_splits(R, U)
    rps = -(-R // nsplit)
    return -(-R // rps)


# R = 1 / 17: the single-row tail alone and behind two 8-row steps; 513 = two default splits of 257 + 256 rows (R one
# more than a split: the second is ragged); 33 rows in 4 splits of 9, 9, 9, 6; 9 rows asked in 4 splits run as 3 x 3
@pytest.mark.parametrize("R,U,nsplit", [(1, 64, None), (17, 64, None), (513, 64, None), (33, 96, 4), (9, 32, 4),
                                        (48, 4096, None)])
def test_kernel_against_float64_segment_sum(R, U, nsplit):
    S, D = 32, 32
    dY, idx = _inputs(R, U, S, D, seed=R)
    gW = torch.zeros(U, S * D, device="cuda")
    _run(dY, idx, D, gW, nsplit)
    if (R, nsplit) == (513, None):
        assert _splits(R, U) == 2
    _check(gW, dY, idx, D, torch.zeros_like(gW), _splits(R, U, nsplit))


def test_all_rows_in_one_class_and_untouched_columns():
    """The longest segment (every step forwards the running sum of the row before); the other classes' columns of a
    non-zero gW keep their bits."""
    S, D, R, U = 32, 32, 300, 64
    dY, _ = _inputs(R, U, S, D, seed=3)
    idx = torch.full((R, S), 5, dtype=torch.int32, device="cuda")
    gW0 = torch.randn(U, S * D, device="cuda") + 3.0
    gW = gW0.clone()
    _run(dY, idx, D, gW)
    _check(gW, dY, idx, D, gW0, _splits(R, U))
    other = torch.ones(S * D, dtype=torch.bool, device="cuda")
    other[torch.arange(S, device="cuda") * D + 5] = False
    assert torch.equal(gW[:, other], gW0[:, other])


def test_strided_views_onto_nonzero_gradient():
    S, D, De, R, U = 32, 32, 48, 70, 96
    dYb, idx = _inputs(R, U + 6, S, D, seed=4)
    dY = dYb[:, 2:U + 2]  # row pitch U + 6, 8-byte aligned start
    full0 = torch.randn(U, S * D + De, device="cuda")
    full = full0.clone()
    _run(dY, idx, D, full[:, :S * D])  # ldw = S*D + De
    _check(full[:, :S * D], dY, idx, D, full0[:, :S * D], _splits(R, U))
    assert torch.equal(full[:, S * D:], full0[:, S * D:])


def test_row_range_of_a_larger_index_buffer():
    S, D, U = 32, 32, 64
    dYb, idxb = _inputs(100, U, S, D, seed=5)
    dY, idx = dYb[30:71], idxb[30:71]
    gW = torch.zeros(U, S * D, device="cuda")
    _run(dY, idx, D, gW)
    _check(gW, dY, idx, D, torch.zeros_like(gW), _splits(41, U))


def test_small_groups_and_unsupported_width_takes_dense_path():
    from dv3hip import engine as E
    from dv3hip import ops

    S, D, R = 4, 4, 37
    dY, idx = _inputs(R, 16, S, D, seed=6)
    gW = torch.zeros(16, S * D, device="cuda")
    _run(dY, idx, D, gW)
    _check(gW, dY, idx, D, torch.zeros_like(gW), 1)
    # an odd width: not the kernel's (8-byte loads) -- the engine's helper keeps the dense product
    U = 15
    assert not ops.onehot_wgrad_ok(R, U, S, D)
    dY, idx = _inputs(R, U, S, D, seed=7)
    with pytest.raises(ValueError):
        ops.onehot_wgrad(dY, idx, D, torch.zeros(U, S * D, device="cuda"), torch.empty(1 << 16, device="cuda"))
    W = torch.nn.Parameter(torch.zeros(U, S * D, device="cuda"))
    W.grad = torch.zeros_like(W)
    x1 = torch.zeros(R, S * D, device="cuda")
    x1.view(R, S, D).scatter_(2, idx.long().unsqueeze(-1), 1.0)
    E.lin_wgrad_onehot(E.Workspace(torch.device("cuda")), "t", W, dY, idx, D, x1)
    torch.cuda.synchronize()
    # dense product: R terms per element (all but the segment's are exact zeros), one rounding each, the partial sums
    # of at most 8 waves, the add into gW
    ref, mag, _ = _reference(dY, idx, D, torch.zeros_like(W))
    err = np.abs(W.grad.cpu().double().numpy() - ref)
    assert float((err - _gamma(R + 8 + 1) * mag).max()) <= 0.0


def test_two_calls_give_the_same_bits():
    S, D, R, U = 32, 32, 1100, 128  # four splits
    dY, idx = _inputs(R, U, S, D, seed=8)
    a = _run(dY, idx, D, torch.zeros(U, S * D, device="cuda"))
    b = _run(dY, idx, D, torch.zeros(U, S * D, device="cuda"))
    assert _splits(R, U) == 4
    assert torch.equal(a, b)


def test_argument_errors_return_before_any_launch():
    from dv3hip import _lib

    lib = _lib.load()
    x, gw = torch.zeros(64, 64, device="cuda"), torch.zeros(64, 1024, device="cuda")
    i = torch.zeros(64, 32, dtype=torch.int32, device="cuda")
    p = torch.empty(1 << 20, device="cuda")
    ok = (x.data_ptr(), 64, i.data_ptr(), 64, 64, 32, 32, gw.data_ptr(), 1024, p.data_ptr(), p.numel(), 1, None)

    def call(**kw):
        names = ("dY", "ldy", "idx", "R", "U", "S", "D", "gW", "ldw", "part", "cap", "nsplit", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.dv3_onehot_wgrad(*[a[n] for n in names])

    assert call(U=63) == 10001 and call(ldy=63) == 10001 and call(S=30) == 10001 and call(D=64) == 10001
    assert call(ldw=1000) == 10001 and call(cap=1000) == 10001 and call(nsplit=0) == 10001 and call(nsplit=65) == 10001
    assert call(dY=None) == 10001 and call(idx=None) == 10001 and call(part=None) == 10001
    assert call(dY=x.data_ptr() + 4) == 10001
    assert call(R=0) == 0


# ---- engine level: the switch on and off --------------------------------------------------------------------------
# "Every other gradient bit-equal" holds for what the unchanged kernels sum in a fixed order: the Linear weights and
# biases and the data gradients.  LayerNorm scale / shift gradients (csrc/rowops.hip) and the conv stack's parameter
# gradients (csrc/conv.hip) are summed with float atomics in no fixed order: two runs of the SAME path differ in their
# last bits (seen on MI355X: MLP layer 0's LayerNorm scale gradient, 37 rows, switch on against off).  For those the
# tests assert what is reproducible -- every workspace buffer (all operands of those launches: activations, statistics,
# upstream gradients) is bit-equal between the two runs, so the launches ran on the same bits -- and, for the MLP's
# LayerNorm gradients, that the two sums differ by no more than two any-order sums of their terms can.
def _zero(params):
    for p in params:
        p.grad = torch.zeros_like(p)


def _stoch_rows(R, S, D, De, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randint(0, D, (R, S), generator=g, dtype=torch.int32).cuda()
    x1 = torch.zeros(R, S * D, device="cuda")
    x1.view(R, S, D).scatter_(2, idx.long().unsqueeze(-1), 1.0)
    return idx, x1, torch.randn(R, De, generator=g).cuda()


def _snapshot(ws):
    return {k: v.clone() for k, v in ws._b.items() if not k[0].endswith(".ohwg")}


def _same_buffers(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _compare_layer0(on, off, dpre, idx, D, SD):
    """Layer 0's stoch columns: the segment sum within its bound of the float64 product of the DENSE run's operands,
    and of the dense result within the two bounds together; the deter columns bit-equal."""
    R = idx.shape[0]
    ref, mag, rows = _reference(dpre, idx, D, torch.zeros(dpre.shape[1], SD))
    b_on = _gamma(rows + 1 + 1)[None, :] * mag
    b_off = _gamma(R + 8 + 1) * mag  # (the dense product: R terms, at most 8 wave partials, the add into gW)
    e_on = np.abs(on[:, :SD].cpu().double().numpy() - ref)
    assert float((e_on - b_on).max()) <= 0.0
    diff = np.abs(on[:, :SD].cpu().double().numpy() - off[:, :SD].cpu().double().numpy())
    assert float((diff - b_on - b_off).max()) <= 0.0
    assert torch.equal(on[:, SD:], off[:, SD:])


def test_mlp_engine_backward_switch_on_and_off(monkeypatch):
    from dv3hip import engine as E

    S, D, De, U, R, A = 4, 4, 16, 32, 37, 8
    SD = S * D
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(11)
    rnd = lambda *sh: (0.3 * torch.randn(*sh, generator=g)).cuda()
    P = torch.nn.Parameter
    layers = [E.PDenseLN(P(rnd(U, SD + De)), P(rnd(U) + 1.0), P(rnd(U))), E.PDenseLN(P(rnd(U, U)), P(rnd(U) + 1.0), P(rnd(U)))]
    out = E.PLin(P(rnd(A, U)), P(rnd(A)))
    names = ["W0", "g0", "b0", "W1", "g1", "b1", "Wo", "bo"]
    params = [t for L in layers for t in (L.W, L.g, L.b)] + [out.W, out.b]
    idx, x1, x2 = _stoch_rows(R, S, D, De, 12)
    dout = torch.randn(R, A, generator=g).cuda()
    res = {}
    for on in (True, False):
        monkeypatch.setattr(E, "_ONEHOT_WGRAD", on)
        monkeypatch.setattr(E, "_ONEHOT_WGRAD_MIN_WORK", 0)  # (the engines keep products this small dense: not here)
        _zero(params)
        eng = E.MLPEngine("t", E.PMLP(layers, out=out), E.Workspace(dev))
        eng.forward(x1, x2)
        dx1, dx2 = torch.empty(R, SD, device=dev), torch.empty(R, De, device=dev)
        eng.backward(x1, x2, slice(0, R), dout=dout, wgrad=True, dx1=dx1, dx2=dx2, idx=idx, D=D)
        torch.cuda.synchronize()
        took = any(k[0] == "t.ohwg" for k in eng.ws._b)
        res[on] = (dict(zip(names, [p.grad.clone() for p in params])), dx1.clone(), dx2.clone(), _snapshot(eng.ws), took)
    assert res[True][4] and not res[False][4]  # (the switch decides which launch ran)
    gon, goff, bufs = res[True][0], res[False][0], res[False][3]
    _same_buffers(res[True][3], bufs)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
    buf = lambda nm: next(v for k, v in bufs.items() if k[0] == nm).double()
    _compare_layer0(gon["W0"], goff["W0"], buf("t.dpre0").float(), idx, D, SD)
    for nm in ("W1", "Wo", "bo"):
        assert torch.equal(gon[nm], goff[nm]), nm
    for i, dy in ((0, "t.dy0"), (1, "t.dh")):  # LayerNorm scale / shift: R terms each, summed by atomics
        xh = (buf(f"t.pre{i}") - buf(f"t.m{i}")[:, None]) * buf(f"t.r{i}")[:, None]
        for nm, terms in ((f"g{i}", buf(dy) * xh), (f"b{i}", buf(dy))):
            bound = 2.0 * float(_gamma(R + 2)) * terms.abs().sum(0)
            assert bool(((gon[nm].double() - goff[nm].double()).abs() <= bound).all()), nm


def test_conv_decoder_engine_backward_switch_on_and_off(monkeypatch):
    import networks
    from dv3hip import engine as E

    S, D, De, R = 4, 4, 16, 5
    SD = S * D
    assert R * 256 < E._ONEHOT_WGRAD_MIN_WORK  # (what the engines do at this size without the patch below)
    torch.manual_seed(13)
    dec = networks.ConvDecoder(SD + De, depth=2).cuda()
    params = list(dec.parameters())
    idx, x1, x2 = _stoch_rows(R, S, D, De, 14)
    drecon = torch.randn(R, 64, 64, 3, generator=torch.Generator(device="cpu").manual_seed(15)).cuda()
    Eo = dec._linear_layer.weight.shape[0]
    res = {}
    for on in (True, False):
        monkeypatch.setattr(E, "_ONEHOT_WGRAD", on)
        monkeypatch.setattr(E, "_ONEHOT_WGRAD_MIN_WORK", 0)  # (the engines keep products this small dense: not here)
        _zero(params)
        eng = dec.engine
        eng.forward(x1, x2)
        dx1, dx2 = torch.empty(R, SD, device="cuda"), torch.empty(R, De, device="cuda")
        eng.backward(drecon, dx1, dx2, idx=idx, D=D)
        torch.cuda.synchronize()
        res[on] = ({n: p.grad.clone() for n, p in dec.named_parameters()}, dx1.clone(), dx2.clone(), _snapshot(eng.ws))
    gon, goff, bufs = res[True][0], res[False][0], res[False][3]
    _same_buffers(res[True][3], bufs)  # (the conv stack's launches ran on the same bits: see the note above)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
    dh0 = next(v for k, v in bufs.items() if k[0] == "dec.dx0").view(R, Eo)
    _compare_layer0(gon["_linear_layer.weight"], goff["_linear_layer.weight"], dh0, idx, D, SD)
    assert torch.equal(gon["_linear_layer.bias"], goff["_linear_layer.bias"])
