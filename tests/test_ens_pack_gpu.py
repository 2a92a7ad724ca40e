"""ops.ens_pack_rows (csrc/ensops.hip, dv3_ens_pack_rows): up to three row-strided sources side by side into a
row-strided destination in one launch, bit-equal to torch.cat of the same views -- contiguous sources (the 16-byte
path where widths and addresses allow it), column / row slices of larger buffers (row stride > width, bases that are
4-byte but not 16-byte aligned), a destination that is itself a column slice, an absent source, rejected arguments,
and capture in a hipGraph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 257)  # one row; fewer rows than a wave; more than one workgroup at every width set
WIDTHS = ((5, 7, 0), (32, 512, 6), (3, 1, 2))  # no multiple of 4 + an absent source; vector-wide + a tail; tiny
SENTINEL = -7.0


def _sources(M, widths, sliced, seed=0):
    """-> list of [M, w] views (None for w == 0).  sliced: each one a row AND column slice of a larger buffer, starting
    at row 1 and column 1 or 2 (whichever leaves the base address off a 16-byte boundary), so that ld > w."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i, w in enumerate(widths):
        if w == 0:
            out.append(None)
        elif sliced:
            big = torch.randn(M + 2, w + 5, device="cuda", generator=gen)
            c0 = 1 if (w + 5 + 1) % 4 else 2
            out.append(big[1:M + 1, c0:c0 + w])
        else:
            out.append(torch.randn(M, w, device="cuda", generator=gen))
    return out


def _expect(srcs):
    return torch.cat([s for s in srcs if s is not None], 1)


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("M", ROWS)
def test_pack_is_torch_cat(M, widths, sliced):
    from dv3hip import ops

    srcs = _sources(M, widths, sliced)
    if sliced:
        assert all(s is None or (s.data_ptr() % 16 != 0 and (M == 1 or s.stride(0) > s.shape[1])) for s in srcs)
    dst = torch.full((M, sum(widths)), SENTINEL, device="cuda")
    assert ops.ens_pack_rows(dst, *srcs) is dst
    torch.cuda.synchronize()
    assert torch.equal(dst, _expect(srcs))


@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("col0", [4, 3], ids=["dst16", "dst4"])
def test_destination_is_a_column_slice(M, widths, col0):
    """dst = wide[:, col0 : col0 + W]: nothing outside the slice is written (col0 3: the slice starts off a 16-byte
    boundary, every source takes the dword path)."""
    from dv3hip import ops

    W = sum(widths)
    srcs = _sources(M, widths, sliced=False, seed=1)
    wide = torch.full((M, W + 12 + (-W) % 4), SENTINEL, device="cuda")  # (row stride: a multiple of 4 floats)
    ops.ens_pack_rows(wide[:, col0:col0 + W], *srcs)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, col0:col0 + W], _expect(srcs))
    assert (wide[:, :col0] == SENTINEL).all() and (wide[:, col0 + W:] == SENTINEL).all()


def test_absent_sources_in_any_slot_and_fewer_than_three():
    from dv3hip import ops

    M = 9
    a, b = torch.randn(M, 8, device="cuda"), torch.randn(M, 3, device="cuda")
    empty = torch.empty(M, 0, device="cuda")
    for srcs in ((a, b), (a,), (None, a, b), (a, empty, b), (empty, None, b)):
        ref = _expect([s for s in srcs if s is not None and s.shape[1]])
        dst = torch.full(ref.shape, SENTINEL, device="cuda")
        ops.ens_pack_rows(dst, *srcs)
        assert torch.equal(dst, ref), [None if s is None else tuple(s.shape) for s in srcs]


def test_wrong_arguments_raise_and_launch_nothing():
    from dv3hip import ops

    M = 6
    a, b = torch.randn(M, 5, device="cuda"), torch.randn(M, 7, device="cuda")
    dst = torch.full((M, 12), SENTINEL, device="cuda")
    ops.PROFILE.start()
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst, a, b[:, :6])  # widths do not add up to dst's
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst[:, :11], a, b)
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst, a, b[:5])  # row counts differ
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst[:5], a, b)
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst, a.t().contiguous().t(), b)  # inner stride is not 1
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst, a.view(M, 5, 1), b)  # not 2-D
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst, a[:, :4], b[:, :4], a[:, :2], b[:, :2])  # more than three sources
    with pytest.raises(ValueError):
        ops.ens_pack_rows(dst)
    with pytest.raises(TypeError):
        ops.ens_pack_rows(dst, a.double(), b)
    with pytest.raises(TypeError):
        ops.ens_pack_rows(dst, a.cpu(), b)
    assert ops.PROFILE.stop() == {}  # no launch was issued
    assert (dst == SENTINEL).all()


def test_library_rejects_bad_strides_before_launching():
    """The C entry's own checks (DV3_ERR_ARG = 10001, nothing launched): ld < w, a missing pointer, negative sizes."""
    from dv3hip import _lib

    lib = _lib.load()
    a = torch.randn(4, 8, device="cuda")
    dst = torch.full((4, 8), SENTINEL, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    pa, pd = a.data_ptr(), dst.data_ptr()
    assert lib.dv3_ens_pack_rows(pa, 7, 8, None, 0, 0, None, 0, 0, pd, 8, 4, stream) == 10001  # ld0 < w0
    assert lib.dv3_ens_pack_rows(pa, 8, 8, None, 0, 0, None, 0, 0, pd, 7, 4, stream) == 10001  # ld_dst < width sum
    assert lib.dv3_ens_pack_rows(None, 8, 8, None, 0, 0, None, 0, 0, pd, 8, 4, stream) == 10001
    assert lib.dv3_ens_pack_rows(pa, 8, 8, None, 0, 0, None, 0, 0, None, 8, 4, stream) == 10001
    assert lib.dv3_ens_pack_rows(pa, 8, -1, None, 0, 0, None, 0, 0, pd, 8, 4, stream) == 10001
    assert lib.dv3_ens_pack_rows(pa, 8, 8, None, 0, 0, None, 0, 0, pd, 8, -1, stream) == 10001
    assert lib.dv3_ens_pack_rows(pa, 8, 8, None, 0, 0, None, 0, 0, pd, 8, 0, stream) == 0  # no rows: nothing to do
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()


def test_captured_in_a_graph_and_replayed_onto_changed_sources():
    from dv3hip import ops

    M, widths = 257, (32, 512, 6)
    big = torch.randn(M + 1, 40, device="cuda")
    srcs = [big[1:, 3:35], torch.randn(M, 512, device="cuda"), torch.randn(M, 6, device="cuda")]
    dst = torch.zeros(M, sum(widths), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ens_pack_rows(dst, *srcs)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ens_pack_rows(dst, *srcs)
    for seed in (1, 2):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        big.copy_(torch.randn(big.shape, device="cuda", generator=gen))
        for s in srcs[1:]:
            s.copy_(torch.randn(s.shape, device="cuda", generator=gen))
        dst.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, _expect(srcs)), seed
