"""Float64 and exact-integer parity of the convolution kernels (csrc/conv.hip) at the edges of their host dispatch.

Every comparison is HIP launches called through dv3hip.ops against a plain float64 PyTorch expression of the same
operation on the CPU: F.conv2d(F.pad(x, [1, 1, 1, 1]), w, None, 2) or F.conv_transpose2d(x, w, bias, 2, padding=1)
+ out_add; input and weight gradients are torch.autograd's on that expression.  Inputs are seeded fp32 tensors cast to
float64 for the reference, so both sides see the same numbers.  Outputs are prefilled with NaN and must be finite
afterwards; accumulated outputs (y under accumulate=True, dw always) are prefilled with seeded non-zero values and the
reference adds to them.  The `dt` argument of the reference functions exists so that the same expression can be
evaluated in fp32 on the CPU: that is how the fp32 oracle's own error against float64 was measured for the bars below
(never from a kernel).

Each case runs twice:
  * randn: weights scaled by 1 / sqrt(fan_in), dy unscaled, held to 1e-4 * max(1, max |ref|) by check(); nothing is
    excluded;
  * int: x, w, dy, bias and the prefilled y / dw are integers in [-3, 3] stored as fp32, out_add = 0.5, and the
    result must EQUAL the float64 reference.  Every product is an integer of magnitude <= 9 and every partial sum of
    any subset of them, plus prefill, bias and out_add, stays below 2^23 (asserted below the tables, on the CPU, from
    the reduction lengths alone), so every summation order -- MFMA chains, split-K atomics, two-stage reductions --
    gives the same bits, and one missing border tap, halo pixel or reduction row is a non-zero difference.

A `conv` row runs ops.conv_s2_fwd, and unless it is forward-only its input gradient (ops.convT_s2_fwd with the same
weight packed transposed=True) and its weight gradient (ops.conv_s2_wgrad); a `convT` row is the mirror image.  Every
forward and data-gradient launch runs with accumulate False and True; every weight gradient is called twice into the
same prefilled dw and must give dw0 + g, then dw0 + 2 g (the packed scratch ops.conv_s2_wgrad caches per dw was
cleared by the unpack kernel, and every path adds).

What each group pins (the gaps tests/test_kernels_gpu.py leaves open):
  A  conv_s2_fwd: the XCD remap of conv_s2_l16_kernel<.., TR=false> (tiles_m % 8 == 0) on 64x64 / 64x96 / 64x128
     tiles, an 8-row last tile, the 128-row tiles 128x128 and 128x96 at their threshold of 448 and the 64-row tile one
     step under it, accumulate=True on the l16, register-direct and k-major paths, the fall-back for a 4-byte-aligned x
     or wp (direct<4>, k-major C64), direct<2> / <4> ragged in every dimension, k-major C64 at 64 < Co <= 128,
     k-major C128 (tiles128 > 256), k-major C128x32;
  B  convT_s2_fwd: the 16 x 16 tile kernel at Co = 1, non-square, with and without bias; l16 with non-power-of-two
     IH, IW (the division branch of rowoff); l16 128x128 / 128x96 at the threshold; l16 64x64, 64x96, 128x32;
     direct<2>, <4>, <8>; k-major C128x32, C64, C128; the 4-byte-aligned fall-back to direct<8>;
  C  weight gradients: the tile walk (32, 64) with G = 3 and 7 (tail loop of the 4-way reduce), non-square, and capped
     at G = 256 by 272 tiles (the register prefetch `tile + gridDim.x < tiles`); the 3-channel tile walk above its cap
     of 512 at both widths; the general path with splits >= 8 (xcd_group = 1, split count padded to a multiple of 8,
     padding workgroups return early), a ragged last chunk, Cfine = 3 off the tile shape, C32x64S / C64 / C128K32;
     dw += on every path and the cleared scratch;
  D  conv_s2_c3_fwd at a ragged grid (45 output pixels), convT_s2_c3_fwd on the scalar kernel (IH % 16 != 0) and on
     the MFMA form at a non-square grid, with bias=None and accumulate; im2col_s2 above its cap of 4096 blocks (second
     trip of the loop); pack_conv_weight in both layouts, ragged and above its cap of 2048 blocks;
  E  a CPU self-check: a pure-Python COPY of the dispatch conditions of dv3_conv_s2_fwd, dv3_convT_s2_fwd and
     dv3_conv_s2_wgrad / ops.conv_s2_wgrad maps every launch of A-C to a path label; each row must land where it
     claims, and the union of the labels must be every path the shipped library can reach.  The copy must be updated
     together with the dispatch thresholds in csrc/conv.hip.

Out of scope (reachable only through development-build switches; DV3_ENV_INT is a constant unless the library is built
with build.py --dev): conv_s2_direct_kernel<8> (DV3_CONV_DIRECT), conv_s2_c3_kernel (DV3_C3_MFMA=0), the serial l16
loop and epilogue variants (DV3_L16_LOOP / DV3_L16_EPI), DV3_WGRAD_K32=0 (conv_wgrad_kernel<C128>).

Bars: 1e-4 * max(1, max |ref|) (TOL of tests/test_kernels_gpu.py, check() of tests/test_row_kernels_f64_gpu.py) for
every float comparison, the weight gradients included.  No bar here is widened: on every case below the fp32 CPU
oracle's own error against float64 stays under half the bar (measured with the same reference functions at
dt=float32).  Worst measured oracle error / bar per group:
  A 0.016 (dw of conv (65,4,8,32,128)), B 0.005 (dw of convT (2,8,8,32,112)),
  C 0.025 (dw of (129,64,64,3,96)), D 0.004 (convT c3 (1,4,12), CW = 96).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_row_kernels_f64_gpu import check, dev, gen

TOL = 1e-4
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
KINDS = ["randn", "int"]
OUT_ADD = 0.5


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


# ============================================================================== E: the dispatch, copied from conv.hip
def cdiv(a, b):
    return -(-a // b)


def conv_path(N, H, W, Ci, Co, aligned=True):
    """dv3_conv_s2_fwd -> (label, tiles_m of the l16 grid or None).  aligned: x and w_packed both 16-byte aligned."""
    M = N * (H // 2) * (W // 2)
    tiles128 = cdiv(M, 128) * cdiv(Co, 128)
    if Ci % 32 == 0 and Co >= 64 and aligned:
        bn = 128 if Co % 128 == 0 else 96 if Co % 96 == 0 else 64
        big = bn != 64 and cdiv(M, 128) * (Co // bn) >= 448
        bm = 128 if big else 64
        return f"l16_{bm}x{bn}", cdiv(M, bm)
    if Ci % 4 == 0 and Co <= 64:  # DV3_CONV_DIRECT = 64 in the shipped library: direct<8> is never taken
        return ("direct2" if Co <= 32 else "direct4"), None
    if Co <= 32:
        return "kmajor_C128x32", None
    if Co <= 64 or tiles128 <= 256:
        return "kmajor_C64", None
    return "kmajor_C128", None


def convT_path(N, IH, IW, Ci, Co, aligned=True):
    """dv3_convT_s2_fwd -> (label, tiles_m of the l16 grid or None)."""
    M = N * IH * IW
    if Co <= 32 and Ci in (16, 32, 48, 64) and IH % 16 == 0 and IW % 16 == 0:
        return "tile16", None
    co96 = Co % 96 == 0 and Co % 128 != 0
    if Ci % 32 == 0 and (Co >= 128 or co96) and aligned:
        bn = 128 if Co % 128 == 0 else 96 if co96 else 64 if Co % 64 == 0 else 32
        big = bn in (128, 96) and cdiv(M, 128) * (Co // bn) * 4 >= 448
        bm = 128 if (bn == 32 or big) else 64
        return f"l16_{bm}x{bn}", cdiv(M, bm)
    if Ci % 4 == 0 and Co <= 128:
        return ("direct2" if Co <= 32 else "direct4" if Co <= 64 else "direct8"), None
    if Co <= 32:
        return "kmajor_C128x32", None
    if Co <= 64:
        return "kmajor_C64", None
    return "kmajor_C128", None


def wgrad_path(N, H, W, Cf, Cc):
    """ops.conv_s2_wgrad + dv3_conv_s2_wgrad / dv3_conv_s2_wgrad_tile -> (label, info).  H, W: the fine grid.
    info: G (workgroups of a tile walk) and tiles, or splits / gsplits (grid rounds of 8) / chunk / last (rows of the
    last split) / xcd of the general split-K path."""
    rows = N * (H // 2) * (W // 2)
    if Cf == 32 and Cc == 64 and H % 16 == 0 and W % 16 == 0:
        tiles = N * (H // 16) * (W // 16)
        return "tile_32x64", {"tiles": tiles, "G": min(tiles, 256)}
    if Cf == 3 and Cc in (32, 96) and (H // 2) % 16 == 0 and (W // 2) % 16 == 0:
        tiles = N * (H // 32) * (W // 32)
        return f"c3tile_{Cc}", {"tiles": tiles, "G": min(tiles, 512)}
    if Cc >= 128:
        name, bm, bn, bk = "C128K32", 128, 128, 32
        target = max(cdiv(Cc, bm) * cdiv(16 * Cf, bn) * cdiv(rows, 3072), 512)
    elif Cc <= 32:
        name, bm, bn, bk, target = "C32x64S", 32, 64, 64, 1024
    else:
        name, bm, bn, bk, target = "C64", 64, 64, 32, 1024
    tiles = cdiv(Cc, bm) * cdiv(16 * Cf, bn)
    splits = max(1, min(cdiv(target, tiles), cdiv(rows, 512)))
    chunk = cdiv(cdiv(rows, splits), bk) * bk
    splits = cdiv(rows, chunk)
    xcd = splits >= 8
    gsplits = cdiv(splits, 8) * 8 if xcd else splits
    return name + ("_c3" if Cf == 3 else ""), {"tiles": tiles, "splits": splits, "gsplits": gsplits, "chunk": chunk,
                                               "last": rows - (splits - 1) * chunk, "xcd": xcd}


def convT_c3_path(N, IH, IW, CW):
    return "mfma" if IH % 16 == 0 and IW % 16 == 0 else "scalar"


CONV_PATHS = {"l16_128x128", "l16_64x128", "l16_128x96", "l16_64x96", "l16_64x64", "direct2", "direct4",
              "kmajor_C128x32", "kmajor_C64", "kmajor_C128"}
CONVT_PATHS = {"tile16", "l16_128x128", "l16_64x128", "l16_128x96", "l16_64x96", "l16_64x64", "l16_128x32",
               "direct2", "direct4", "direct8", "kmajor_C128x32", "kmajor_C64", "kmajor_C128"}
WGRAD_PATHS = {"tile_32x64", "c3tile_32", "c3tile_96", "C128K32", "C128K32_c3", "C32x64S", "C32x64S_c3", "C64", "C64_c3"}

# ================================================================================================== the case tables
# (path the forward launch must take, (N, H, W, Ci, Co), "fdw" | "f" (forward only), None | "x+wp" (4-byte-aligned
#  bases: x first, then wp), claims about the l16 grid)
CONV_ROWS = [
    ("l16_64x64", (2, 32, 32, 32, 72), "fdw", None, {"tiles_m": 8}),    # remap, ragged Co (two column tiles, 8 live)
    ("l16_64x96", (2, 32, 32, 32, 192), "fdw", None, {"tiles_m": 8}),
    ("l16_64x128", (4, 32, 32, 32, 128), "fdw", None, {"tiles_m": 16}),
    ("l16_64x128", (65, 4, 8, 32, 128), "fdw", None, {"tiles_m": 9}),   # M = 520: 8-row last tile, no remap
    ("l16_64x128", (111, 32, 32, 32, 256), "f", None, {"tiles_m": 444}),  # 222 x 2 = 444 < 448
    ("l16_128x128", (28, 64, 64, 32, 256), "f", None, {"tiles_m": 224}),  # 224 x 2 = 448
    ("l16_128x96", (28, 64, 64, 32, 192), "f", None, {"tiles_m": 224}),   # 224 x 2 = 448
    ("direct4", (2, 8, 8, 32, 64), "f", "x+wp", {}),
    ("kmajor_C64", (2, 8, 8, 32, 128), "f", "x+wp", {}),
    ("direct4", (13, 4, 10, 12, 40), "fdw", None, {}),    # M = 130: two workgroups, the second with 2 rows
    ("direct2", (5, 12, 4, 36, 17), "fdw", None, {}),
    ("kmajor_C64", (2, 8, 8, 16, 100), "fdw", None, {}),
    ("kmajor_C128", (33, 64, 64, 16, 128), "f", None, {}),  # tiles128 = 264 > 256
    # not in the dispatch-edge list, here so that E's union is whole: the k-major 128x32 tile of both dispatchers
    # (the data gradient of this row is convT 18 -> 6 channels, Ci % 4 != 0), two row tiles
    ("kmajor_C128x32", (5, 12, 10, 6, 18), "fdw", None, {}),
]
# (path, (N, IH, IW, Ci, Co), "fdw" | "f", None | "x" (4-byte-aligned x), claims, also with bias=None)
CONVT_ROWS = [
    ("tile16", (1, 16, 32, 48, 1), "f", None, {}, True),
    ("l16_64x128", (2, 6, 10, 32, 128), "fdw", None, {"tiles_m": 2}, False),   # rowoff by division
    ("l16_128x128", (14, 32, 32, 32, 128), "f", None, {"tiles_m": 112}, False),  # 112 x 1 x 4 = 448
    ("l16_128x96", (14, 32, 32, 32, 96), "f", None, {"tiles_m": 112}, False),    # 112 x 1 x 4 = 448
    ("l16_64x64", (2, 4, 4, 32, 320), "fdw", None, {"tiles_m": 1}, False),
    ("direct8", (3, 6, 6, 20, 100), "fdw", None, {}, False),
    ("direct8", (2, 8, 8, 32, 112), "fdw", None, {}, False),
    ("kmajor_C64", (3, 5, 3, 6, 40), "fdw", None, {}, False),
    ("kmajor_C128", (2, 4, 6, 48, 160), "fdw", None, {}, False),
    ("direct8", (2, 4, 4, 32, 128), "f", "x", {}, False),
    # not in the dispatch-edge list, here so that E's union is whole
    ("l16_64x96", (3, 6, 6, 32, 96), "f", None, {"tiles_m": 2}, False),   # 2 x 1 x 4 = 8 < 448
    ("l16_128x32", (5, 6, 6, 32, 160), "f", None, {"tiles_m": 2}, False),
    ("direct4", (5, 6, 6, 12, 40), "f", None, {}, False),
]
# (path, (N, H, W, Cfine, Ccoarse) with H, W the fine grid, claims)
WGRAD_ROWS = [
    ("tile_32x64", (3, 16, 16, 32, 64), {"G": 3}),
    ("tile_32x64", (7, 16, 16, 32, 64), {"G": 7}),
    ("tile_32x64", (1, 16, 48, 32, 64), {"G": 3}),
    ("tile_32x64", (17, 64, 64, 32, 64), {"tiles": 272, "G": 256}),
    ("c3tile_32", (129, 64, 64, 3, 32), {"tiles": 516, "G": 512}),
    ("c3tile_96", (129, 64, 64, 3, 96), {"tiles": 516, "G": 512}),
    # rows = 18 * 16 * 16 = 4608; 1 x 4 tiles of 128 x 128; target max(4 * ceil(4608 / 3072), 512) = 512 workgroups ->
    # 128 splits, capped at ceil(4608 / 512) = 9; chunk = ceil(4608 / 9) = 512 (a multiple of BK = 32); 9 splits, the
    # grid has 16 (7 padding splits x 4 tiles return early)
    ("C128K32", (18, 32, 32, 32, 128), {"splits": 9, "gsplits": 16, "chunk": 512, "last": 512, "xcd": True}),
    # rows = 29 * 16 * 10 = 4640; cap ceil(4640 / 512) = 10; chunk = ceil(4640 / 10) = 464 -> 480 (BK = 32);
    # ceil(4640 / 480) = 10 splits, the last with 4640 - 9 * 480 = 320 rows
    ("C128K32", (29, 32, 20, 32, 128), {"splits": 10, "gsplits": 16, "chunk": 480, "last": 320, "xcd": True}),
    # rows = 32 * 12 * 12 = 4608 (12 % 16 != 0: not the tile walk); 1 x 1 tile of 32 x 64 (48 live columns); target
    # 1024 -> capped at 9; chunk 512 (a multiple of BK = 64); 9 splits
    ("C32x64S_c3", (32, 24, 24, 3, 32), {"splits": 9, "gsplits": 16, "chunk": 512, "xcd": True}),
    # rows = 4608; 1 x 2 tiles; 1024 / 2 = 512 -> capped at 9; chunk 512; 9 splits
    ("C32x64S", (18, 32, 32, 8, 16), {"splits": 9, "gsplits": 16, "chunk": 512, "xcd": True}),
    # rows = 4608; 1 x 4 tiles of 64 x 64; 1024 / 4 = 256 -> capped at 9; chunk 512; 9 splits
    ("C64", (18, 32, 32, 16, 64), {"splits": 9, "gsplits": 16, "chunk": 512, "xcd": True}),
    # not in the dispatch-edge list, here so that E's union is whole: 3 fine channels at the other widths
    ("C64_c3", (2, 8, 8, 3, 40), {"splits": 1, "xcd": False}),
    ("C128K32_c3", (2, 8, 8, 3, 128), {"splits": 1, "xcd": False}),
]
C3_CONV_SHAPES = [(3, 6, 10)]                                  # (N, H, W): 45 output pixels, one partly filled block
C3_CONVT_SHAPES = [(2, 8, 8), (1, 4, 12), (1, 16, 48)]         # (N, IH, IW): scalar, scalar, MFMA
C3_WIDTHS = [32, 96]


def _launches():
    """Every (dispatcher, shape, aligned) that the rows of A-C launch, with the reduction length of each output."""
    out = []
    for _, (N, H, W, Ci, Co), mode, align, _ in CONV_ROWS:
        out.append(("conv", (N, H, W, Ci, Co), align is None, 16 * Ci))
        if mode == "fdw":
            out.append(("convT", (N, H // 2, W // 2, Co, Ci), True, 4 * Co))
            out.append(("wgrad", (N, H, W, Ci, Co), True, N * (H // 2) * (W // 2)))
    for _, (N, IH, IW, Ci, Co), mode, align, _, _ in CONVT_ROWS:
        out.append(("convT", (N, IH, IW, Ci, Co), align is None, 4 * Ci))
        if mode == "fdw":
            out.append(("conv", (N, 2 * IH, 2 * IW, Co, Ci), True, 16 * Co))
            out.append(("wgrad", (N, 2 * IH, 2 * IW, Co, Ci), True, N * IH * IW))
    for _, (N, H, W, Cf, Cc), _ in WGRAD_ROWS:
        out.append(("wgrad", (N, H, W, Cf, Cc), True, N * (H // 2) * (W // 2)))
    return out


# Exactness of the integer runs is a property of the inputs: |x w| <= 9 per term, K terms, + prefill (3) + bias (3) +
# out_add (0.5); a weight gradient is added twice into its prefill.  Half-integers below 2^23 are exact in fp32.
for _op, _shape, _, _K in _launches():
    assert 9 * (2 * _K if _op == "wgrad" else _K) + 7 < 2 ** 23, (_op, _shape, _K)
for _CW in C3_WIDTHS:
    assert 9 * max(48, 4 * _CW) + 7 < 2 ** 23


def test_every_case_lands_on_its_path_and_every_path_has_a_case():
    """E.  conv_path / convT_path / wgrad_path above are a COPY of the conditions in dv3_conv_s2_fwd, dv3_convT_s2_fwd
    and dv3_conv_s2_wgrad / ops.conv_s2_wgrad (shipped library: every DV3_ENV_INT at its default); they must be
    updated together with the dispatch thresholds.  Each row lands on the path it claims, with the grid it claims, and
    the launches of this file together reach every path of the three dispatchers."""
    for path, shape, _, align, claims in CONV_ROWS:
        got, tiles_m = conv_path(*shape, aligned=align is None)
        assert got == path, (shape, got, path)
        assert claims.get("tiles_m", tiles_m) == tiles_m, (shape, tiles_m)
        if align is not None:  # the aligned call of the same shape would have taken the l16 tile
            assert conv_path(*shape)[0].startswith("l16_")
    for path, shape, _, align, claims, _ in CONVT_ROWS:
        got, tiles_m = convT_path(*shape, aligned=align is None)
        assert got == path, (shape, got, path)
        assert claims.get("tiles_m", tiles_m) == tiles_m, (shape, tiles_m)
        if align is not None:
            assert convT_path(*shape)[0].startswith("l16_")
    for path, shape, claims in WGRAD_ROWS:
        got, info = wgrad_path(*shape)
        assert got == path, (shape, got, path)
        for k, v in claims.items():
            assert info[k] == v, (shape, k, info[k], v)
    # the edges the row comments name
    assert conv_path(2, 32, 32, 32, 72)[1] % 8 == 0 and conv_path(65, 4, 8, 32, 128)[1] % 8 != 0
    assert 65 * 2 * 4 - 8 * 64 == 8
    info = wgrad_path(29, 32, 20, 32, 128)[1]
    assert 0 < info["last"] < info["chunk"] and info["gsplits"] > info["splits"]
    seen = {"conv": set(), "convT": set(), "wgrad": set()}
    grouped = set()
    for op, shape, aligned, _ in _launches():
        if op == "wgrad":
            label, info = wgrad_path(*shape)
            grouped.add(info.get("xcd"))
        else:
            label = (conv_path if op == "conv" else convT_path)(*shape, aligned=aligned)[0]
        seen[op].add(label)
    assert seen["conv"] == CONV_PATHS, seen["conv"] ^ CONV_PATHS
    assert seen["convT"] == CONVT_PATHS, seen["convT"] ^ CONVT_PATHS
    assert seen["wgrad"] == WGRAD_PATHS, seen["wgrad"] ^ WGRAD_PATHS
    assert {True, False} <= grouped
    assert {convT_c3_path(*s, 32) for s in C3_CONVT_SHAPES} == {"scalar", "mfma"}


# ====================================================================================================== references
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def ref_conv(x, w, dy=None, dt=F64):
    """Conv2d k4 s2 'same' on NCHW -> (y, dx, dw); the gradients for the upstream dy (None: forward only)."""
    x, w = x.to(dt).requires_grad_(dy is not None), w.to(dt).requires_grad_(dy is not None)
    y = F.conv2d(F.pad(x, [1, 1, 1, 1]), w, None, 2)
    if dy is None:
        return y, None, None
    y.backward(dy.to(dt))
    return y.detach(), x.grad, w.grad


def ref_convT(x, w, bias, out_add, dy=None, dt=F64):
    """ConvTranspose2d k4 s2 p1 + bias + out_add on NCHW -> (y, dx, dw)."""
    x, w = x.to(dt).requires_grad_(dy is not None), w.to(dt).requires_grad_(dy is not None)
    y = F.conv_transpose2d(x, w, None if bias is None else bias.to(dt), 2, padding=1) + out_add
    if dy is None:
        return y, None, None
    y.backward(dy.to(dt))
    return y.detach(), x.grad, w.grad


def ref_wgrad(coarse, fine, dt=F64):
    """Weight gradient [Cc, Cf, 4, 4] of sum(conv(fine) * coarse), NCHW operands."""
    w = torch.zeros(coarse.shape[1], fine.shape[1], 4, 4, dtype=dt, requires_grad=True)
    F.conv2d(F.pad(fine.to(dt), [1, 1, 1, 1]), w, None, 2).backward(coarse.to(dt))
    return w.grad


def ref_im2col(x):
    """x [N, C, H, W] -> cols [N * (H/2) * (W/2), (ci, ky, kx)]."""
    u = F.unfold(F.pad(x, [1, 1, 1, 1]), 4, stride=2)  # [N, C * 16, L]
    return u.transpose(1, 2).reshape(-1, u.shape[1])


def ref_pack(w, transposed):
    """The packed images of ops.pack_conv_weight: Conv2d [Co, Ci, 4, 4] -> [Co, (ky, kx, ci)]; ConvTranspose2d
    [Ci, Co, 4, 4] -> [cls = (py, px), Co, (a, b, ci)] with (ky, kx) = (1 - py + 2 a, 1 - px + 2 b)."""
    if not transposed:
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    Ci, Co = w.shape[0], w.shape[1]
    w6 = w.reshape(Ci, Co, 2, 2, 2, 2).flip(3).flip(5)  # [ci, co, a, py, b, px]
    return w6.permute(3, 5, 1, 2, 4, 0).reshape(4, Co, 4 * Ci)


# ========================================================================================================= helpers
def seed_of(tag, shape, kind):
    s = sum(ord(c) for c in tag) + (977 if kind == "int" else 0)
    for v in shape:
        s = (s * 1009 + int(v)) % (2 ** 31 - 1)
    return s


def draw(shape, kind, g, scale=1.0):
    if kind == "int":
        return torch.randint(-3, 4, tuple(shape), generator=g).to(F32)
    return torch.randn(*shape, generator=g) * scale


def full(shape):
    return torch.full(tuple(shape), NAN, device="cuda")


def off4(t):
    """A contiguous copy of t on the GPU whose base is 4 bytes past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def compare(got, ref, kind, what):
    if kind != "int":
        return check(got, ref, TOL, what)
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bad = int((got != ref).sum())
    print(f"{what}: exact" if bad == 0 else
          f"{what}: {bad} of {ref.numel()} differ, max |diff| {(got - ref).abs().max().item():.3e}")
    assert torch.equal(got, ref), f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"


def run_fwd(launch, ref, kind, g, what):
    """launch(y, accumulate) with y NaN-filled and accumulate=False, then with a seeded prefill and accumulate=True."""
    for acc in (False, True):
        y0 = draw(ref.shape, kind, g) if acc else None
        y = dev(y0) if acc else full(ref.shape)
        launch(y, acc)
        compare(y, ref + y0.double() if acc else ref, kind, f"{what}{' accumulate' if acc else ''}")


def run_wgrad(ops, coarse, fine, g_ref, kind, g, what):
    """dw prefilled; two calls into the same dw: dw0 + g, then dw0 + 2 g."""
    dw0 = draw(g_ref.shape, kind, g)
    dw = dev(dw0)
    for k in (1, 2):
        ops.conv_s2_wgrad(coarse, fine, dw)
        compare(dw, dw0.double() + k * g_ref, kind, f"{what} call {k}")


def conv_inputs(shape, kind, mode):
    N, H, W, Ci, Co = shape
    g = gen(seed_of("conv", shape, kind))
    x = draw((N, Ci, H, W), kind, g)
    w = draw((Co, Ci, 4, 4), kind, g, 1.0 / math.sqrt(16 * Ci))
    dy = draw((N, Co, H // 2, W // 2), kind, g) if mode == "fdw" else None
    return g, x, w, dy


def convT_inputs(shape, kind, mode):
    N, IH, IW, Ci, Co = shape
    g = gen(seed_of("convT", shape, kind))
    x = draw((N, Ci, IH, IW), kind, g)
    w = draw((Ci, Co, 4, 4), kind, g, 1.0 / math.sqrt(4 * Ci))
    b = draw((Co,), kind, g)
    dy = draw((N, Co, 2 * IH, 2 * IW), kind, g) if mode == "fdw" else None
    return g, x, w, b, dy


def wgrad_inputs(shape, kind):
    N, H, W, Cf, Cc = shape
    g = gen(seed_of("wgrad", shape, kind))
    return g, draw((N, Cc, H // 2, W // 2), kind, g), draw((N, Cf, H, W), kind, g)


def row_id(row):
    return f"{row[0]}-{'x'.join(str(v) for v in row[1])}"


# ================================================================================================== A: conv_s2_fwd
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", CONV_ROWS, ids=row_id)
def test_conv_s2_rows(ops, row, kind):
    path, shape, mode, align, _ = row
    N, H, W, Ci, Co = shape
    g, x, w, dy = conv_inputs(shape, kind, mode)
    y_ref, dx_ref, dw_ref = ref_conv(x, w, dy)
    xd, wd = dev(nhwc(x)), dev(w)
    wp = torch.empty(Co, 16 * Ci, device="cuda")
    ops.pack_conv_weight(wd, wp, transposed=False)
    what = f"conv {shape} {kind} {path}"
    if align is None:
        run_fwd(lambda y, acc: ops.conv_s2_fwd(xd, wp, y, Ci=Ci, Co=Co, accumulate=acc), nhwc(y_ref), kind, g, what)
    else:
        xo, wo = off4(xd), off4(wp)
        run_fwd(lambda y, acc: ops.conv_s2_fwd(xo, wp, y, Ci=Ci, Co=Co, accumulate=acc), nhwc(y_ref), kind, g,
                what + " x at 4 bytes")
        run_fwd(lambda y, acc: ops.conv_s2_fwd(xd, wo, y, Ci=Ci, Co=Co, accumulate=acc), nhwc(y_ref), kind, g,
                what + " wp at 4 bytes")
    if mode != "fdw":
        return
    # input gradient: ConvTranspose2d with the Conv2d weight read as [in = Co][out = Ci]
    dyd = dev(nhwc(dy))
    wpt = torch.empty(4, Ci, 4 * Co, device="cuda")
    ops.pack_conv_weight(wd, wpt, transposed=True)
    run_fwd(lambda o, acc: ops.convT_s2_fwd(dyd, wpt, o, Ci=Co, Co=Ci, accumulate=acc), nhwc(dx_ref), kind, g,
            f"{what} dgrad ({convT_path(N, H // 2, W // 2, Co, Ci)[0]})")
    run_wgrad(ops, dyd, xd, dw_ref, kind, g, f"{what} wgrad ({wgrad_path(N, H, W, Ci, Co)[0]})")


# ================================================================================================= B: convT_s2_fwd
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", CONVT_ROWS, ids=row_id)
def test_convT_s2_rows(ops, row, kind):
    path, shape, mode, align, _, also_no_bias = row
    N, IH, IW, Ci, Co = shape
    g, x, w, b, dy = convT_inputs(shape, kind, mode)
    y_ref, dx_ref, dw_ref = ref_convT(x, w, b, OUT_ADD, dy)
    xd, wd, bd = dev(nhwc(x)), dev(w), dev(b)
    wpt = torch.empty(4, Co, 4 * Ci, device="cuda")
    ops.pack_conv_weight(wd, wpt, transposed=True)
    xin = xd if align is None else off4(xd)
    what = f"convT {shape} {kind} {path}" + ("" if align is None else " x at 4 bytes")
    run_fwd(lambda y, acc: ops.convT_s2_fwd(xin, wpt, y, Ci=Ci, Co=Co, bias=bd, out_add=OUT_ADD, accumulate=acc),
            nhwc(y_ref), kind, g, what)
    if also_no_bias:
        run_fwd(lambda y, acc: ops.convT_s2_fwd(xin, wpt, y, Ci=Ci, Co=Co, out_add=OUT_ADD, accumulate=acc),
                nhwc(y_ref - b.double().view(1, -1, 1, 1)), kind, g, what + " bias=None")
    if mode != "fdw":
        return
    # input gradient: Conv2d over dOut with the ConvTranspose2d weight read as [out = Ci][in = Co]
    dyd = dev(nhwc(dy))
    wp = torch.empty(Ci, 16 * Co, device="cuda")
    ops.pack_conv_weight(wd, wp, transposed=False)
    run_fwd(lambda o, acc: ops.conv_s2_fwd(dyd, wp, o, Ci=Co, Co=Ci, accumulate=acc), nhwc(dx_ref), kind, g,
            f"{what} dgrad ({conv_path(N, 2 * IH, 2 * IW, Co, Ci)[0]})")
    run_wgrad(ops, xd, dyd, dw_ref, kind, g, f"{what} wgrad ({wgrad_path(N, 2 * IH, 2 * IW, Co, Ci)[0]})")


# ============================================================================================= C: weight gradients
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", WGRAD_ROWS, ids=row_id)
def test_conv_wgrad_rows(ops, row, kind):
    path, shape, _ = row
    g, coarse, fine = wgrad_inputs(shape, kind)
    run_wgrad(ops, dev(nhwc(coarse)), dev(nhwc(fine)), ref_wgrad(coarse, fine), kind, g, f"wgrad {shape} {kind} {path}")


# ================================================================================= D: image-side and layout kernels
def c3_conv_inputs(shape, CW, kind):
    N, H, W = shape
    g = gen(seed_of("c3conv", shape + (CW,), kind))
    return g, draw((N, 3, H, W), kind, g), draw((CW, 3, 4, 4), kind, g, 1.0 / math.sqrt(48))


def c3_convT_inputs(shape, CW, kind):
    N, IH, IW = shape
    g = gen(seed_of("c3convT", shape + (CW,), kind))
    return g, draw((N, CW, IH, IW), kind, g), draw((CW, 3, 4, 4), kind, g, 1.0 / math.sqrt(4 * CW)), draw((3,), kind, g)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CW", C3_WIDTHS)
@pytest.mark.parametrize("shape", C3_CONV_SHAPES)
def test_conv_s2_c3(ops, shape, CW, kind):
    g, x, w = c3_conv_inputs(shape, CW, kind)
    y_ref = nhwc(ref_conv(x, w)[0])
    xd, wd = dev(nhwc(x)), dev(w)
    run_fwd(lambda y, acc: ops.conv_s2_c3_fwd(xd, wd, y, CW=CW, accumulate=acc), y_ref, kind, g,
            f"conv c3 {shape} CW {CW} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CW", C3_WIDTHS)
@pytest.mark.parametrize("shape", C3_CONVT_SHAPES)
def test_convT_s2_c3(ops, shape, CW, kind):
    g, x, w, b = c3_convT_inputs(shape, CW, kind)
    xd, wd, bd = dev(nhwc(x)), dev(w), dev(b)
    y_ref = nhwc(ref_convT(x, w, b, OUT_ADD)[0])
    what = f"convT c3 {shape} CW {CW} {kind} {convT_c3_path(*shape, CW)}"
    run_fwd(lambda y, acc: ops.convT_s2_c3_fwd(xd, wd, y, CW=CW, bias=bd, out_add=OUT_ADD, accumulate=acc), y_ref,
            kind, g, what)
    run_fwd(lambda y, acc: ops.convT_s2_c3_fwd(xd, wd, y, CW=CW, out_add=OUT_ADD, accumulate=acc),
            y_ref - b.double().view(1, 1, 1, 3), kind, g, what + " bias=None")


@pytest.mark.gpu
def test_im2col_s2_above_the_grid_cap(ops):
    """5 x 16 x 16 x 1024 = 1,310,720 elements against 4096 blocks x 256 threads: the second trip of the loop."""
    N, H, W, C = 5, 32, 32, 64
    assert N * (H // 2) * (W // 2) * 16 * C > 4096 * 256
    x = torch.randn(N, C, H, W, generator=gen(11))
    cols = full((N * (H // 2) * (W // 2), 16 * C))
    ops.im2col_s2(dev(nhwc(x)), cols)
    assert torch.equal(cols.cpu(), ref_im2col(x))


@pytest.mark.gpu
@pytest.mark.parametrize("Co,Ci", [(7, 5), (384, 192)])
@pytest.mark.parametrize("transposed", [False, True])
def test_pack_conv_weight(ops, transposed, Co, Ci):
    """Both packed layouts, ragged and above the cap of 2048 blocks x 256 threads (16 x 384 x 192 = 1,179,648)."""
    w = torch.randn((Ci, Co, 4, 4) if transposed else (Co, Ci, 4, 4), generator=gen(Co + Ci))
    wp = full((4, Co, 4 * Ci) if transposed else (Co, 16 * Ci))
    ops.pack_conv_weight(dev(w), wp, transposed=transposed)
    assert torch.equal(wp.cpu(), ref_pack(w, transposed))
