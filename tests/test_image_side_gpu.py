"""The 3-channel image-side kernels: the forward conv (encoder layer 0, the decoder's last layer's data gradient) on its
band kernel and its fall-backs, and the transposed conv (the decoder's last layer) on its 8 x 16 input tiles.

dv3_conv_s2_c3_fwd takes conv_s2_c3_band_kernel when the output rows divide a 128-pixel tile (OW 16, 32 or 64, OH a
multiple of 128 / OW) and x and y are 16-byte aligned, and conv_s2_c3_mfma_kernel (any pixel count, 128-pixel tiles
that straddle rows and images) otherwise.  `path()` below is a copy of that condition: THE COPY MUST BE UPDATED WITH
csrc/conv.hip.  Cases, at CW 32 and 96:
  band   one tile exactly (16x32 frame: R = 8 output rows of 16), all three row widths (OW 16, 32, 64), the non-square
         32x64 and 64x32 frames, several tiles per image and several images (the tile -> (image, row band) split, the
         band's first row above the image at oy0 = 0 and its last row below it at the bottom tile, the zero pixels left
         and right of every row: all four borders), accumulate on and off;
  mfma   a frame whose rows do not fill tiles (20x64: OH = 10, R = 4), a ragged grid (6x6 frames, 45 output pixels),
         and the band shape with x or y four bytes off a 16-byte boundary.
Every case against a float64 conv2d on the CPU with the bar 1e-4 * max(1, max |ref|) of tests/test_row_kernels_f64_gpu.py
(tests/test_conv_f64_gpu.py: the fp32 oracle's own error stays under half of it at these K = 48 sums); with small
integers and half-integers every product and partial sum is exact in fp32 and the result must be EQUAL; two runs of
the same inputs are bit-identical (no atomics in a forward kernel), and the band kernel's result is bit-identical to
the 128-pixel-tile kernel's on the same data (same products, same k order), which the misaligned cases check.

dv3_convT_s2_c3_fwd takes convT_s2_c3_mfma_kernel when IH and IW are multiples of 16 (`convT_path`, as in
tests/test_conv_f64_gpu.py) and the thread-per-pixel kernel otherwise.  The MFMA kernel's workgroup owns 8 input rows x
16 columns plus a one-pixel halo, so: two row tiles with nothing beside them (16x16: the halo above, below, left and
right is all outside the image), tiles with neighbours on every side (32x32, 16x48, 32x16: the halo is the neighbour's
pixels), several images; with bias and without, out_add = 0.5, accumulate on and off, exact integers, two runs equal.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_row_kernels_f64_gpu import check, dev, gen

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
WIDTHS = [32, 96]
# (N, H, W)
BAND_SHAPES = [(1, 16, 32), (2, 32, 32), (3, 64, 64), (2, 32, 64), (2, 64, 32), (2, 8, 128), (1, 4, 128)]
MFMA_SHAPES = [(2, 20, 64), (5, 6, 6), (3, 6, 10), (1, 2, 2)]
# (N, IH, IW) of the transposed conv
CONVT_SHAPES = [(1, 16, 16), (3, 32, 32), (2, 16, 48), (2, 32, 16), (2, 8, 8), (1, 4, 12)]
OUT_ADD = 0.5


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def path(N, H, W, aligned=True):
    OW, OH = W // 2, H // 2
    return "band" if aligned and OW in (16, 32, 64) and OH % (128 // OW) == 0 else "mfma"


def test_shapes_land_on_the_paths_they_name():
    assert all(path(*s) == "band" for s in BAND_SHAPES) and all(path(*s) == "mfma" for s in MFMA_SHAPES)
    assert {s[2] // 2 for s in BAND_SHAPES} == {16, 32, 64}
    assert any(s[0] * (s[1] // 2) * (s[2] // 2) == 128 for s in BAND_SHAPES)  # one tile exactly
    assert any((s[1] // 2) * (s[2] // 2) > 128 and s[0] > 1 for s in BAND_SHAPES)  # tiles per image > 1, images > 1
    assert any(s[0] * (s[1] // 2) * (s[2] // 2) == 45 for s in MFMA_SHAPES)


def inputs(shape, CW, kind):
    N, H, W = shape
    g = gen(N * 1000003 + H * 10007 + W * 101 + CW + (7 if kind == "int" else 0))
    if kind == "int":  # small integers and half-integers: every partial sum is exact in fp32
        x = torch.randint(-4, 5, (N, H, W, 3), generator=g).to(F32) * 0.5
        w = torch.randint(-3, 4, (CW, 3, 4, 4), generator=g).to(F32) * 0.5
        y0 = torch.randint(-8, 9, (N, H // 2, W // 2, CW), generator=g).to(F32) * 0.5
    else:
        x = torch.randn(N, H, W, 3, generator=g)
        w = torch.randn(CW, 3, 4, 4, generator=g) * 0.3
        y0 = torch.randn(N, H // 2, W // 2, CW, generator=g)
    return x, w, y0


def ref_conv(x, w):
    """Conv2d k4 s2 'same' (rows 2 oy - 1 + ky): float64 on the CPU, NHWC in and out."""
    return F.conv2d(x.to(F64).permute(0, 3, 1, 2), w.to(F64), stride=2, padding=1).permute(0, 2, 3, 1).contiguous()


def run(ops, xd, wd, y0, CW, accumulate, ybuf=None):
    y = ybuf if ybuf is not None else torch.empty_like(y0, device="cuda")
    y.copy_(y0 if accumulate else torch.full_like(y0, float("nan")))
    ops.conv_s2_c3_fwd(xd, wd, y, CW=CW, accumulate=accumulate)
    return y


@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("CW", WIDTHS)
@pytest.mark.parametrize("shape", BAND_SHAPES + MFMA_SHAPES)
def test_conv_s2_c3_fwd(ops, shape, CW, kind):
    x, w, y0 = inputs(shape, CW, kind)
    ref = ref_conv(x, w)
    xd, wd = dev(x), dev(w)
    what = f"conv c3 {shape} CW {CW} {kind} {path(*shape)}"
    for acc in (False, True):
        want = ref + y0.to(F64) if acc else ref
        got = run(ops, xd, wd, y0, CW, acc)
        if kind == "int":
            assert torch.equal(got.cpu().double(), want), f"{what} acc {acc}: exact-integer run differs"
        else:
            check(got, want, what=f"{what} acc {acc}")
        assert torch.equal(got, run(ops, xd, wd, y0, CW, acc)), f"{what} acc {acc}: two runs differ"


@pytest.mark.parametrize("CW", WIDTHS)
@pytest.mark.parametrize("which", ["x", "y"])
def test_misaligned_operand_takes_the_tile_kernel_and_agrees_bit_for_bit(ops, CW, which):
    """x or y four bytes off a 16-byte boundary: the band kernel's vector accesses are not possible, the 128-pixel-tile
    kernel runs -- and, computing the same products in the same order, returns the same bits."""
    shape = (3, 64, 64)
    x, w, y0 = inputs(shape, CW, "randn")
    xd, wd = dev(x), dev(w)
    assert xd.data_ptr() % 16 == 0
    for acc in (False, True):
        band = run(ops, xd, wd, y0, CW, acc)
        if which == "x":
            xo = torch.empty(x.numel() + 1, device="cuda")[1:].view(x.shape)
            xo.copy_(xd)
            assert xo.data_ptr() % 16 == 4
            tile = run(ops, xo, wd, y0, CW, acc)
        else:
            yo = torch.empty(y0.numel() + 1, device="cuda")[1:].view(y0.shape)
            assert yo.data_ptr() % 16 == 4
            tile = run(ops, xd, wd, y0, CW, acc, ybuf=yo)
        check(tile, ref_conv(x, w) + (y0.to(F64) if acc else 0), what=f"conv c3 misaligned {which} CW {CW} acc {acc}")
        assert torch.equal(band, tile), f"band and tile kernels differ (CW {CW}, {which} misaligned, acc {acc})"


# ------------------------------------------------------------------------------------------------ transposed conv
def convT_path(N, IH, IW):
    return "mfma" if IH % 16 == 0 and IW % 16 == 0 else "scalar"


def test_convT_shapes_cover_both_kernels():
    assert [convT_path(*s) for s in CONVT_SHAPES] == ["mfma"] * 4 + ["scalar"] * 2


def convT_inputs(shape, CW, kind):
    N, IH, IW = shape
    g = gen(N * 1000003 + IH * 10007 + IW * 101 + CW + (7 if kind == "int" else 0) + 13)
    if kind == "int":
        x = torch.randint(-4, 5, (N, IH, IW, CW), generator=g).to(F32) * 0.5
        w = torch.randint(-3, 4, (CW, 3, 4, 4), generator=g).to(F32) * 0.5
        b = torch.randint(-3, 4, (3,), generator=g).to(F32) * 0.5
        y0 = torch.randint(-8, 9, (N, 2 * IH, 2 * IW, 3), generator=g).to(F32) * 0.5
    else:
        x = torch.randn(N, IH, IW, CW, generator=g)
        w = torch.randn(CW, 3, 4, 4, generator=g) * 0.3
        b = torch.randn(3, generator=g)
        y0 = torch.randn(N, 2 * IH, 2 * IW, 3, generator=g)
    return x, w, b, y0


def ref_convT(x, w, b):
    """ConvTranspose2d k4 s2 p1 (+ bias + OUT_ADD): float64 on the CPU, NHWC in and out."""
    y = F.conv_transpose2d(x.to(F64).permute(0, 3, 1, 2), w.to(F64), None if b is None else b.to(F64), stride=2, padding=1)
    return (y + OUT_ADD).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("CW", WIDTHS)
@pytest.mark.parametrize("shape", CONVT_SHAPES)
def test_convT_s2_c3_fwd(ops, shape, CW, kind):
    x, w, b, y0 = convT_inputs(shape, CW, kind)
    xd, wd, bd = dev(x), dev(w), dev(b)
    for bias in (b, None):
        ref = ref_convT(x, w, bias)
        for acc in (False, True):
            what = f"convT c3 {shape} CW {CW} {kind} {convT_path(*shape)} bias {bias is not None} acc {acc}"
            want = ref + y0.to(F64) if acc else ref

            def once():
                y = dev(y0) if acc else torch.full_like(y0, float("nan"), device="cuda")
                return ops.convT_s2_c3_fwd(xd, wd, y, CW=CW, bias=None if bias is None else bd, out_add=OUT_ADD,
                                           accumulate=acc)

            got = once()
            if kind == "int":
                assert torch.equal(got.cpu().double(), want), f"{what}: exact-integer run differs"
            else:
                check(got, want, what=what)
            assert torch.equal(got, once()), f"{what}: two runs differ"
