"""The k-contiguous LDS tile engine (gemm_l16_kernel, conv_s2_l16_kernel): software-pipelined K loop, batched epilogue
and the transposed convolution's per-row output decode.

Exact-arithmetic checks: operands are drawn from {-8 .. 8} / 8, so every product is a multiple of 1/64 and every
partial sum up to K = 1536 (|sum| <= 1536, 6 fraction bits: 17 significant bits) is exact in fp32 -- the result must
equal the float64 product cast to fp32 bit for bit, whatever the order of the summation.  A dropped, repeated or raced
K chunk or epilogue element shows up exactly.  Bias, out_add and the accumulate base are multiples of 1/8 as well.

Old loop against new loop: one child process runs the development library with the serial loop and the serial
epilogue selected (DV3_L16_LOOP=0 DV3_L16_EPI=0) on random normal data; the shipped library must give the same bits.

Parent recording: both loops are one piece of shared code (csrc/l16_tile.h), so an error they have in common, or a
changed order of summation, shows only against outputs recorded from the kernels as they were before the loop moved
there (tests/golden/l16_parent*.npz, written by tests/golden/make_l16_parent_control.py)."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L16_TILES = (12, 13, 14, 15, 16, 17)  # 64x96, 64x64, 32x64, 128x128, 128x64, 64x128


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def eighths(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 8.0


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# (K1, K2): nk = 1, 2, odd, even, and the [A | A2] seam on a K-tile boundary
K_CASES = [(32, 0), (64, 0), (96, 0), (512, 0), (32, 64)]


@pytest.mark.parametrize("M,N", [(33, 65), (130, 255), (1024, 1030)])
def test_gemm_l16_exact(ops, M, N):
    g = torch.Generator().manual_seed(M * 7 + N)
    b = eighths(g, N)
    C0 = eighths(g, M, N)
    bd, C0d = b.cuda(), C0.cuda()
    for K1, K2 in K_CASES:
        A, W = eighths(g, M, K1 + K2), eighths(g, N, K1 + K2)
        prod = A.double() @ W.double().t()
        Ad = A.cuda()
        A1d, A2d = (Ad[:, :K1], Ad[:, K1:]) if K2 else (Ad, None)  # column slices of one buffer: lda = K1 + K2
        Wd = W.cuda()
        for acc in (False, True):
            for bias in (False, True):
                want = (prod + (b.double() if bias else 0) + (C0.double() if acc else 0)).float().cuda()
                for tile in L16_TILES:
                    C = C0d.clone()
                    ops.gemm(A1d, Wd, C, A2=A2d, bias=bd if bias else None, accumulate=acc, tile=tile)
                    assert torch.equal(C, want), (
                        f"tile {tile} {M}x{N}x{K1}+{K2} acc {acc} bias {bias}: "
                        f"{int((C != want).sum())} elements differ, max {float((C - want).abs().max()):.3e}")


@pytest.mark.parametrize("M,N,n1", [(33, 65, 16), (130, 255, 64), (1024, 1030, 512)])
def test_gemm_l16_split_output_exact(ops, M, N, n1):
    """[C | C2] with accumulate2 != accumulate: each destination keeps its own flag and its own row stride."""
    g = torch.Generator().manual_seed(M + N + n1)
    C0, D0 = eighths(g, M, n1), eighths(g, M, N - n1)
    for K in (32, 96, 512):
        A, W = eighths(g, M, K), eighths(g, N, K)
        prod = A.double() @ W.double().t()
        for acc, acc2 in ((True, False), (False, True)):
            C, C2 = C0.cuda(), D0.cuda()
            ops.gemm_split(A.cuda(), W.cuda(), C, C2, accumulate=acc, accumulate2=acc2)
            want = (prod[:, :n1] + (C0.double() if acc else 0)).float().cuda()
            want2 = (prod[:, n1:] + (D0.double() if acc2 else 0)).float().cuda()
            assert torch.equal(C, want), f"C {M}x{N}x{K} split {n1} acc {acc}/{acc2}"
            assert torch.equal(C2, want2), f"C2 {M}x{N}x{K} split {n1} acc {acc}/{acc2}"


def test_gemm_l16_sampling_tile_exact(ops):
    """The 32 x 64 tile with the sampling epilogue (EPI = 1): exact logits, and the sample of exactly those logits."""
    M, N = 1030, 1024
    g = torch.Generator().manual_seed(11)
    b = eighths(g, N).cuda()
    q = torch.empty(M, N // 32, 32).exponential_(1.0, generator=g).clamp_min(1e-20).cuda()
    for K in (32, 64, 96, 512):
        A, W = eighths(g, M, K), eighths(g, N, K)
        want = (A.double() @ W.double().t() + b.cpu().double()).float().cuda()
        lg, st = torch.empty(M, N, device="cuda"), torch.empty(M, N // 32, 32, device="cuda")
        idx = torch.empty(M * N // 32, dtype=torch.int32, device="cuda")
        ops.gemm_sample(A.cuda(), W.cuda(), lg, st, bias=b, noise=q, idx=idx)
        assert torch.equal(lg, want), f"logits K {K}: {int((lg != want).sum())} elements differ"
        st0, idx0 = torch.empty_like(st), torch.empty_like(idx)
        ops.onehot_sample(want.view(M, N // 32, 32), st0, noise=q, idx=idx0)
        assert torch.equal(st, st0) and torch.equal(idx, idx0), f"sample K {K}"


def conv_case(ops, g, Nimg, H, W, Ci, Co, acc, rnd=eighths):
    x, w = rnd(g, Nimg, Ci, H, W), rnd(g, Co, Ci, 4, 4)
    y0 = rnd(g, Nimg, H // 2, W // 2, Co)
    wp = torch.empty(Co, 16 * Ci, device="cuda")
    ops.pack_conv_weight(w.cuda(), wp, transposed=False)
    y = y0.cuda()
    ops.conv_s2_fwd(nhwc(x).cuda(), wp, y, Ci=Ci, Co=Co, accumulate=acc)
    want = nhwc(F.conv2d(F.pad(x.double(), [1, 1, 1, 1]), w.double(), None, 2)) + (y0.double() if acc else 0)
    return y, want.float().cuda()


def convT_case(ops, g, Nimg, H, W, Ci, Co, acc, rnd=eighths):
    x, w, b = rnd(g, Nimg, Ci, H, W), rnd(g, Ci, Co, 4, 4), rnd(g, Co)
    y0 = rnd(g, Nimg, 2 * H, 2 * W, Co)
    wp = torch.empty(4, Co, 4 * Ci, device="cuda")
    ops.pack_conv_weight(w.cuda(), wp, transposed=True)
    y = y0.cuda()
    ops.convT_s2_fwd(nhwc(x).cuda(), wp, y, Ci=Ci, Co=Co, bias=b.cuda(), out_add=0.5, accumulate=acc)
    want = nhwc(F.conv_transpose2d(x.double(), w.double(), b.double(), 2, padding=1)) + 0.5 + (y0.double() if acc else 0)
    return y, want.float().cuda()


# the last of each: a spatial size that is no power of two (the epilogue's general row decode)
@pytest.mark.parametrize("Nimg,H,W,Ci,Co", [(3, 8, 8, 32, 64), (3, 8, 8, 32, 96), (3, 12, 12, 32, 64), (2, 12, 20, 32, 128)])
@pytest.mark.parametrize("acc", [False, True])
def test_conv_s2_l16_exact(ops, Nimg, H, W, Ci, Co, acc):
    g = torch.Generator().manual_seed(Nimg + H + Ci + Co)
    y, want = conv_case(ops, g, Nimg, H, W, Ci, Co, acc)
    assert torch.equal(y, want), f"{int((y != want).sum())} elements differ, max {float((y - want).abs().max()):.3e}"


# 3 x 4 x 4: M = 48 rows per parity class on a 64-row tile; 64 -> 64 at 8 x 8; Co 96: the 64 x 96 tile
@pytest.mark.parametrize("Nimg,H,W,Ci,Co", [(3, 4, 4, 32, 128), (3, 8, 8, 64, 64), (3, 4, 4, 32, 96), (3, 6, 6, 32, 128),
                                          (2, 3, 5, 32, 128)])
@pytest.mark.parametrize("acc", [False, True])
def test_convT_s2_l16_exact(ops, Nimg, H, W, Ci, Co, acc):
    g = torch.Generator().manual_seed(Nimg + H + Ci + Co)
    y, want = convT_case(ops, g, Nimg, H, W, Ci, Co, acc)
    assert torch.equal(y, want), f"{int((y != want).sum())} elements differ, max {float((y - want).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------ old loop against new loop
def ab_outputs(ops):
    """Random normal data through every l16 tile and the two conv cases: name -> output (same seeds in both processes)."""
    g = torch.Generator().manual_seed(2024)
    randn = lambda g_, *s: torch.randn(*s, generator=g_)
    out = {}
    for M, N, K1, K2, acc in ((1024, 1536, 512, 512, False), (1024, 1030, 512, 0, True), (256, 255, 512, 0, False)):
        K = K1 + K2
        A, W = randn(g, M, K).cuda(), (randn(g, N, K) / math.sqrt(K)).cuda()
        b, C0 = randn(g, N).cuda(), randn(g, M, N).cuda()
        A1, A2 = (A[:, :K1], A[:, K1:]) if K2 else (A, None)
        for tile in L16_TILES:
            C = C0.clone()
            ops.gemm(A1, W, C, A2=A2, bias=b, accumulate=acc, tile=tile)
            out[f"gemm {M}x{N}x{K1}+{K2} tile {tile}"] = C
    for acc in (False, True):
        out[f"conv acc {acc}"] = conv_case(ops, g, 3, 8, 8, 32, 64, acc, rnd=randn)[0]
        out[f"conv96 acc {acc}"] = conv_case(ops, g, 3, 8, 8, 32, 96, acc, rnd=randn)[0]
        out[f"convT acc {acc}"] = convT_case(ops, g, 3, 4, 4, 32, 128, acc, rnd=randn)[0]
        out[f"convT64 acc {acc}"] = convT_case(ops, g, 3, 8, 8, 64, 64, acc, rnd=randn)[0]
    torch.cuda.synchronize()
    return out


def test_serial_loop_of_the_development_library_gives_the_same_bits(ops, tmp_path):
    dev_lib = os.path.join(REPO, "dreamerv3-torch_amd", "dv3hip", "libdv3hip_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (builds libdv3hip_dev.so as well)"
    path = str(tmp_path / "serial.pt")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DV3")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path],
                       env=dict(env, DV3HIP_LIB=dev_lib, DV3_L16_LOOP="0", DV3_L16_EPI="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    old = torch.load(path)
    new = ab_outputs(ops)
    assert sorted(old) == sorted(new)
    for name, t in new.items():
        assert torch.equal(t.cpu(), old[name]), f"{name}: {int((t.cpu() != old[name]).sum())} elements differ"


# ------------------------------------------------------------------------------------------ parent recording
def test_l16_matches_parent_recording(ops):
    """Random normal data, the smallest shapes that reach every phase of the loop (nk = 1, 2, 3, the [A | A2] seam) and
    an edge tile on every tile shape: every bit as the parent commit computed it.  Not covered here: the 128-row conv
    tiles (chosen from 448 workgroups up: tests/test_fullsize_gpu.py) and the sampling tile
    (test_gemm_l16_sampling_tile_exact)."""
    from tests.golden import make_l16_parent_control as parent  # (not at module level: the child process below)

    path = os.path.join(REPO, "tests", "golden", "l16_parent.npz")
    rec = parent.load(path)
    for tile in parent.L16_TILES:
        for name, C in parent.gemm_cases(ops, rec, tile).items():
            assert torch.equal(C.cpu(), rec[name]), f"{name} tile {tile}: {int((C.cpu() != rec[name]).sum())} elements differ"
    for name, C in parent.split_case(ops, rec).items():
        assert torch.equal(C.cpu(), rec[name]), f"{name}: {int((C.cpu() != rec[name]).sum())} elements differ"
    rec = parent.load(parent.conv_path(path))
    for name, y in parent.conv_cases(ops, rec).items():
        assert torch.equal(y.cpu(), rec[name]), f"{name}: {int((y.cpu() != rec[name]).sum())} elements differ"


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "dreamerv3-torch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from dv3hip import _dev, ops as _ops

    assert _dev.enabled(), "the child needs the development library (DV3HIP_LIB)"
    torch.save({k: v.cpu() for k, v in ab_outputs(_ops).items()}, sys.argv[1])
