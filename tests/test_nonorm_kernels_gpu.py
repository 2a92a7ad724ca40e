"""Float64 parity of the LayerNorm-free row kernels (csrc/rowops.hip: dv3_act_fwd / dv3_act_bwd, dv3_gru_nonorm_fwd /
_fwd_blend / _bwd), in the style and at the bar of tests/test_row_kernels_f64_gpu.py.

Every comparison is one HIP kernel, called through dv3hip.ops, against a plain float64 PyTorch expression of the same
operation on the CPU; gradients are torch.autograd's on that expression.  Inputs are seeded fp32 tensors cast to float64
for the reference, so both sides see the same numbers.  Bar: 1e-4 * max(1, max|ref|).

What the shapes pin:
  * act: 1x1; 3x5 (scalar kernel, ragged tail of the last workgroup); 77x16 and 2x2048 (16-byte kernel, short and long
    rows); WRAP x 4 with WRAP = ACT_GRID_CAP * 256 + 3 rows of one chunk each and WRAP / 3 rows of 3 floats (second trip
    of the grid-stride loop in the 16-byte and in the scalar kernel);
    row strides of N + 4 on x / y / dy / dx with the padding checked untouched; a base pointer that is not 16-byte
    aligned (the scalar kernel at N % 4 == 0); the (C,H,W) flatten with 16 pixels per image at N = 3 and N = 16;
    accumulate_dx on and off, dx in place of dy; +-20 and +-50 for saturation; ReLU inputs at least 1e-3 from zero
    (its derivative jumps there);
  * GRU: De = 3 (scalar), 16, 256, 1024, 2048 x M = 1, 3, 17; the fused next-step reset blend at the widths
    dv3_gru_fwd_blend takes, with next_first all zeros / all ones / mixed, and its refusal at the others; accumulate_dh
    on and off, dh in place of dh'; pre-activations within +-10, and +-40 where the gates saturate and everything must
    stay finite.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4
F32, F64 = torch.float32, torch.float64
ACTS = ["none", "SiLU", "ReLU", "ELU", "GELU", "Tanh", "Mish"]
REF_ACT = {"none": lambda z: z * 1.0, "SiLU": F.silu, "ReLU": F.relu, "ELU": F.elu, "GELU": F.gelu, "Tanh": torch.tanh,
           "Mish": F.mish}


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def check(got, ref, tol=TOL, what="", floor=1.0):
    """max |got - ref| <= tol * max(floor, max |ref|)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    bar = tol * max(floor, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"{what}: max err {err:.3e} bar {bar:.3e}")
    assert err <= bar, f"{what}: max err {err:.3e} > bar {bar:.3e}"


def off_zero(x):
    """Every element at least 1e-3 from zero (the sign is kept)."""
    return torch.where(x.abs() < 1e-3, torch.where(x < 0, -1e-3, 1e-3).to(x.dtype), x)


def act_inputs(R, N, seed, saturate=False):
    g = gen(seed)
    x = 2 * torch.randn(R, N, generator=g)
    if saturate:
        lv = torch.tensor([20.0, -20.0, 50.0, -50.0])
        x = torch.where(torch.rand(R, N, generator=g) < 0.5, lv[torch.randint(0, 4, (R, N), generator=g)], x)
    return off_zero(x), torch.randn(R, N, generator=g), torch.randn(R, N, generator=g)


def ref_act(x, dy, act):
    """-> (act(x), dy * act'(x)) in float64."""
    xd = x.double().requires_grad_(True)
    y = REF_ACT[act](xd)
    (dx,) = torch.autograd.grad(y, xd, dy.double())
    return y.detach(), dx


def padded(t, pad, fill=-7.0):
    """A CUDA copy of t [R, N] as a view with row stride N + pad; -> (view, whole buffer)."""
    R, N = t.shape
    buf = torch.full((R, N + pad), fill, dtype=F32, device="cuda")
    buf[:, :N] = t.cuda()
    return buf[:, :N], buf


def wrap_rows(ops, N=4):
    """Rows of N columns that take the kernel into the second trip of its grid-stride loop: more than ACT_GRID_CAP * 256
    chunks of 16 bytes (N = 4: one per row) or, in the scalar kernel (N = 3), floats."""
    per_row = 1 if N % 4 == 0 else N
    return ops.ACT_GRID_CAP * 256 // per_row + 3


# ------------------------------------------------------------------------------------------------ act_fwd / act_bwd
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (77, 16), (2, 2048), ("wrap", 4), ("wrap", 3)], ids=str)
@pytest.mark.parametrize("act", ACTS)
def test_act_fwd_bwd(ops, act, shape):
    R, N = shape
    if R == "wrap":
        R = wrap_rows(ops, N)
    x, dy, dx0 = act_inputs(R, N, seed=100 + N)
    y_ref, dx_ref = ref_act(x, dy, act)
    xg, dyg = x.cuda(), dy.cuda()
    y = torch.empty_like(xg)
    assert ops.act_fwd(xg, y, act=act) is y
    check(y, y_ref, what=f"act_fwd {act} {R}x{N}")
    dx = torch.full_like(xg, float("nan"))
    ops.act_bwd(dyg, xg, dx, act=act)
    check(dx, dx_ref, what=f"act_bwd {act} {R}x{N}")
    dx = dx0.cuda()
    ops.act_bwd(dyg, xg, dx, act=act, accumulate_dx=True)
    check(dx, dx0.double() + dx_ref, what=f"act_bwd += {act} {R}x{N}")
    ops.act_bwd(dyg, xg, dyg, act=act)  # in place
    check(dyg, dx_ref, what=f"act_bwd in place {act} {R}x{N}")


@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("act", ACTS)
def test_act_saturated_inputs(ops, act, N):
    x, dy, _ = act_inputs(77, N, seed=7, saturate=True)
    assert (x.abs() == 50).any() and (x.abs() == 20).any()
    y_ref, dx_ref = ref_act(x, dy, act)
    y, dx = torch.empty(77, N, device="cuda"), torch.empty(77, N, device="cuda")
    ops.act_fwd(x.cuda(), y, act=act)
    ops.act_bwd(dy.cuda(), x.cuda(), dx, act=act)
    check(y, y_ref, what=f"act_fwd saturated {act} N={N}")
    check(dx, dx_ref, what=f"act_bwd saturated {act} N={N}")


@pytest.mark.parametrize("R,N", [(3, 5), (77, 16), ("wrap", 4)])
@pytest.mark.parametrize("act", ["SiLU", "ELU"])
def test_act_row_strides(ops, act, R, N):
    """ld = N + 4 on every operand; the four padding columns of the outputs keep their contents."""
    if R == "wrap":
        R = wrap_rows(ops)
    x, dy, dx0 = act_inputs(R, N, seed=31)
    y_ref, dx_ref = ref_act(x, dy, act)
    xv, _ = padded(x, 4)
    dyv, _ = padded(dy, 4)
    yv, ybuf = padded(torch.zeros(R, N), 4)
    ops.act_fwd(xv, yv, act=act)
    check(yv, y_ref, what=f"act_fwd strided {act} {R}x{N}")
    assert (ybuf[:, N:] == -7.0).all()
    for acc in (False, True):
        dxv, dxbuf = padded(dx0, 4)
        ops.act_bwd(dyv, xv, dxv, act=act, accumulate_dx=acc)
        check(dxv, dx_ref + (dx0.double() if acc else 0), what=f"act_bwd strided acc={acc} {act} {R}x{N}")
        assert (dxbuf[:, N:] == -7.0).all()


@pytest.mark.parametrize("act", ["SiLU", "Tanh"])
def test_act_unaligned_base_takes_the_scalar_kernel(ops, act):
    """N % 4 == 0 but the tensors start 4 bytes past a 16-byte boundary: same results, nothing outside the tensors."""
    R, N = 9, 16
    x, dy, _ = act_inputs(R, N, seed=5)
    y_ref, dx_ref = ref_act(x, dy, act)

    def shifted(t):
        buf = torch.full((R * N + 8,), -7.0, dtype=F32, device="cuda")
        v = buf[1:1 + R * N].view(R, N)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v, buf

    xv, _ = shifted(x)
    dyv, _ = shifted(dy)
    yv, ybuf = shifted(torch.zeros(R, N))
    dxv, dxbuf = shifted(torch.zeros(R, N))
    ops.act_fwd(xv, yv, act=act)
    ops.act_bwd(dyv, xv, dxv, act=act)
    check(yv, y_ref, what=f"act_fwd unaligned {act}")
    check(dxv, dx_ref, what=f"act_bwd unaligned {act}")
    for buf in (ybuf, dxbuf):
        assert buf[0] == -7.0 and (buf[1 + R * N:] == -7.0).all()


@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("act", ["SiLU", "ReLU", "Mish"])
def test_act_chw_group(ops, act, N):
    """chw_group = 16: rows are (image, pixel) pairs and y / dy are the (C,H,W) flatten of each image."""
    G, imgs = 16, 3
    R = imgs * G
    x, dy_chw, dx0 = act_inputs(R, N, seed=11)

    def to_chw(t):  # [R, N] rows -> [imgs, N * G] with (c, pix) order
        return t.view(imgs, G, N).transpose(1, 2).reshape(imgs, N * G)

    def from_chw(t):
        return t.view(imgs, N, G).transpose(1, 2).reshape(R, N)

    dy_rows = from_chw(dy_chw.view(imgs, N * G))
    y_ref, dx_ref = ref_act(x, dy_rows, act)
    xg = x.cuda()
    y = torch.empty(imgs, N * G, device="cuda")
    ops.act_fwd(xg, y, act=act, chw_group=G)
    check(y, to_chw(y_ref), what=f"act_fwd chw {act} N={N}")
    dyg = dy_chw.view(imgs, N * G).contiguous().cuda()
    for acc in (False, True):
        dx = dx0.cuda()
        ops.act_bwd(dyg, xg, dx, act=act, chw_group=G, accumulate_dx=acc)
        check(dx, dx_ref + (dx0.double() if acc else 0), what=f"act_bwd chw acc={acc} {act} N={N}")


def test_act_wrappers_check_shapes(ops):
    x = torch.zeros(4, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.act_fwd(x, torch.zeros(4, 7, device="cuda"))
    with pytest.raises(ValueError):
        ops.act_bwd(torch.zeros(3, 8, device="cuda"), x, torch.zeros(4, 8, device="cuda"))
    with pytest.raises(ValueError):
        ops.act_fwd(x, torch.zeros(32, device="cuda"), chw_group=3)  # 4 rows are no whole number of 3-pixel images
    with pytest.raises(NotImplementedError):
        ops.act_fwd(x, torch.zeros(4, 8, device="cuda"), act="Softsign")
    with pytest.raises(TypeError):
        ops.act_fwd(torch.zeros(4, 8), torch.zeros(4, 8))


# ------------------------------------------------------------------------------------------------ GRU without norm
def ref_gru(p, h, g=None, dt=F64):
    """GRUCell.forward with norm=False on the pre-activations p = W cat[x, h]; -> h' (and dp, dh for upstream g)."""
    pd, hd = p.to(dt).requires_grad_(True), h.to(dt).requires_grad_(True)
    r, c, u = pd.chunk(3, -1)
    r = torch.sigmoid(r)
    c = torch.tanh(r * c)
    u = torch.sigmoid(u - 1)
    hn = u * c + (1 - u) * hd
    if g is None:
        return hn.detach()
    dp, dh = torch.autograd.grad(hn, (pd, hd), g.to(dt))
    return hn.detach(), dp, dh


def gru_inputs(M, De, seed, scale=10.0):
    g = gen(seed)
    p = scale * (2 * torch.rand(M, 3 * De, generator=g) - 1)
    return p, torch.tanh(torch.randn(M, De, generator=g)), torch.randn(M, De, generator=g), \
        torch.randn(M, De, generator=g)


def blend_ok(De):
    return (De % 256 == 0 and De <= 1024) or (De % 1024 == 0 and De <= 4096)


@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("De", [3, 16, 256, 1024, 2048])
def test_gru_nonorm_fwd_bwd(ops, De, M):
    p, h, g, dh0 = gru_inputs(M, De, seed=1000 + De + M)
    hn_ref, dp_ref, dh_ref = ref_gru(p, h, g)
    pg, hg, gg = p.cuda(), h.cuda(), g.cuda()
    hn = torch.full((M, De), float("nan"), device="cuda")
    assert ops.gru_nonorm_fwd(pg, hg, hn) is hn
    check(hn, hn_ref, what=f"gru_nonorm_fwd De={De} M={M}")
    for acc in (False, True):
        dp = torch.full((M, 3 * De), float("nan"), device="cuda")
        dh = dh0.cuda()
        ops.gru_nonorm_bwd(gg, pg, hg, dp, dh, accumulate_dh=acc)
        check(dp, dp_ref, what=f"gru_nonorm_bwd dp acc={acc} De={De} M={M}")
        check(dh, dh_ref + (dh0.double() if acc else 0), what=f"gru_nonorm_bwd dh acc={acc} De={De} M={M}")
    dp = torch.empty(M, 3 * De, device="cuda")
    ops.gru_nonorm_bwd(gg, pg, hg, dp, gg)  # dh in place of dh'
    check(dp, dp_ref, what=f"gru_nonorm_bwd dp in place De={De} M={M}")
    check(gg, dh_ref, what=f"gru_nonorm_bwd dh in place De={De} M={M}")


@pytest.mark.parametrize("first", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("De", [256, 1024, 2048])
def test_gru_nonorm_fwd_blend(ops, De, M, first):
    p, h, _, init = gru_inputs(M, De, seed=2000 + De + M)
    init = init[0].contiguous()
    nf = {"zeros": torch.zeros(M), "ones": torch.ones(M), "mixed": (torch.arange(M) % 2 == 0).float()}[first]
    hn_ref = ref_gru(p, h)
    nxt_ref = hn_ref * (1 - nf.double()[:, None]) + init.double()[None] * nf.double()[:, None]
    hn = torch.empty(M, De, device="cuda")
    nxt, nbuf = padded(torch.zeros(M, De), 4)
    ops.gru_nonorm_fwd(p.cuda(), h.cuda(), hn, next_blend=(nf.cuda(), init.cuda(), nxt))
    check(hn, hn_ref, what=f"gru_nonorm_fwd_blend h' De={De} M={M} {first}")
    check(nxt, nxt_ref, what=f"gru_nonorm_fwd_blend next De={De} M={M} {first}")
    assert (nbuf[:, De:] == -7.0).all()


@pytest.mark.parametrize("De", [3, 16])
def test_gru_nonorm_fwd_blend_refuses_other_widths(ops, De):
    from dv3hip._lib import DV3Error

    assert not blend_ok(De)
    p, h, _, init = gru_inputs(3, De, seed=1)
    hn, nxt = torch.empty(3, De, device="cuda"), torch.empty(3, De, device="cuda")
    with pytest.raises(DV3Error):
        ops.gru_nonorm_fwd(p.cuda(), h.cuda(), hn, next_blend=(torch.zeros(3, device="cuda"), init[0].cuda(), nxt))


@pytest.mark.parametrize("De", [3, 256])
def test_gru_nonorm_row_strides(ops, De):
    M = 5
    p, h, g, dh0 = gru_inputs(M, De, seed=77)
    hn_ref, dp_ref, dh_ref = ref_gru(p, h, g)
    pv, _ = padded(p, 4)
    hv, _ = padded(h, 4)
    gv, _ = padded(g, 4)
    hn, hnbuf = padded(torch.zeros(M, De), 4)
    dp, dpbuf = padded(torch.zeros(M, 3 * De), 4)
    dh, dhbuf = padded(dh0, 4)
    ops.gru_nonorm_fwd(pv, hv, hn)
    ops.gru_nonorm_bwd(gv, pv, hv, dp, dh, accumulate_dh=True)
    check(hn, hn_ref, what=f"gru_nonorm_fwd strided De={De}")
    check(dp, dp_ref, what=f"gru_nonorm_bwd strided dp De={De}")
    check(dh, dh_ref + dh0.double(), what=f"gru_nonorm_bwd strided dh De={De}")
    for buf, n in ((hnbuf, De), (dpbuf, 3 * De), (dhbuf, De)):
        assert (buf[:, n:] == -7.0).all()


@pytest.mark.parametrize("De", [3, 256])
def test_gru_nonorm_saturated_gates_stay_finite(ops, De):
    M = 17
    p, h, g, _ = gru_inputs(M, De, seed=9, scale=40.0)
    p = torch.where(p > 0, torch.full_like(p, 40.0), torch.full_like(p, -40.0))
    hn_ref, dp_ref, dh_ref = ref_gru(p, h, g)
    hn, dp, dh = (torch.empty(M, n, device="cuda") for n in (De, 3 * De, De))
    ops.gru_nonorm_fwd(p.cuda(), h.cuda(), hn)
    ops.gru_nonorm_bwd(g.cuda(), p.cuda(), h.cuda(), dp, dh)
    check(hn, hn_ref, what=f"gru_nonorm_fwd saturated De={De}")
    check(dp, dp_ref, what=f"gru_nonorm_bwd saturated dp De={De}")
    check(dh, dh_ref, what=f"gru_nonorm_bwd saturated dh De={De}")


def test_gru_nonorm_wrappers_check_shapes(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError):
        ops.gru_nonorm_fwd(z(4, 47), z(4, 16), z(4, 16))
    with pytest.raises(ValueError):
        ops.gru_nonorm_fwd(z(4, 48), z(4, 16), z(3, 16))
    with pytest.raises(ValueError):
        ops.gru_nonorm_bwd(z(4, 16), z(4, 48), z(4, 16), z(4, 47), z(4, 16))
    with pytest.raises(ValueError):
        ops.gru_nonorm_fwd(z(4, 768), z(4, 256), z(4, 256), next_blend=(z(3), z(256), z(4, 256)))
