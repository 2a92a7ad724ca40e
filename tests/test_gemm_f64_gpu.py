"""Float64 and exact-integer parity of the GEMM engines (csrc/gemm.hip, csrc/mfma_gemm.h) at the edges of their dispatch.

Every comparison is one or more HIP launches through dv3hip.ops (group G: the ctypes library of dv3hip._lib.load())
against a plain float64 PyTorch product on the CPU:

    C0 * [accumulate] + cat([A, A2], -1) @ op(B) + bias

Operands are seeded fp32 tensors cast to float64 for the reference, so both sides see the same numbers.  Overwritten
outputs are prefilled with NaN and must be finite afterwards; accumulated outputs are prefilled with seeded non-zero
values.  Where C is a column window of a wider buffer, the columns outside it must be bit-unchanged.  Row-strided
operands carry 7777 in their padding columns: finite, so that the kernels' "load a safe address, multiply by a zero
mask" idiom stays legal, and far outside the data, so that one padding element used as data is a failure in both runs.
The `dt` argument of reference() exists so that the same expression can be evaluated in fp32 on the CPU: that is how
the fp32 oracle's own error against float64 was measured for the bars below (oracle_ratio(), never from a kernel).

Each case runs twice:
  * randn: the weights scaled by 1 / sqrt(K) (dY by 1 / sqrt(rows) for weight gradients), so that the result is O(1),
    held to 1e-4 * max(1, max |ref|) by check(); nothing is excluded;
  * int: A, A2, B, bias and the prefill are integers in [-3, 3] stored as fp32 and the result must EQUAL the float64
    reference.  Every product is an integer of magnitude <= 9 and every partial sum of any subset of them, plus prefill
    and bias, stays below 2^23 (asserted below the tables, on the CPU, from the largest K alone), so every summation
    order -- MFMA chains in any k order, the wave-group reductions through LDS, split-K atomics -- gives the same bits,
    and one missing, repeated or misplaced element is a non-zero difference.

A case is G(tile, orientation, M, N, K1, K2, ...): orientation "NT" is y = x W^T (transA = 0, transB = 1), "NN" the data
gradient (B as [K][N]), "TN" the weight gradient (A as [K][M], B as [K][N]), "TT" both transposed.  lay: "plain", "odd"
(row-strided views with an odd leading dimension), "off1" (base pointer one float past a 16-byte boundary), "wide4"
(leading dimension + 8: strided but still legal for the k-contiguous LDS tiles).  win: C is a column window.

What each group pins (the gaps tests/test_kernels_gpu.py leaves open):
  A  the k-major LDS engine gemm_kernel<TS, TA, TB>, forced tiles 0, 1, 2, 4, 5, 6, 8, each in all four orientations:
     M, N one under / one over BM, BN, a last tile of one row and one column; K = 3, BK - 1 (tail tile only, n_full = 0),
     BK, BK + 1, 2 BK + 3; bias, accumulate, C as a window, odd leading dimensions and a 4-byte-aligned base (the f32x4u
     loads) in rotation; [A | A2] on NT and NN with K1 = 32 (64 for tiles 5, 6, 8) and K2 = 1, 3, BK, BK + 5; the
     split-K of launch_ts (accumulate, NT / NN / TN, ragged last chunk, bias exactly once, grids of 8 and of 12
     workgroups and one of 28 = 4 tiles x 7 splits: the remainder branch of xcd_remap); the wave-split tiles 6 and 8
     with and without workgroup split-K on top;
  B  the few-row kernels: tile 3 at M = 1 .. 128 and N = 1, 15, 17, 300 in both B layouts and all three accumulate
     modes, register batch depths <3>, <6>, <12> named per row, fewer chunks than waves, a last batch clamped onto the
     last chunk, K % 16 != 0, K % 4 != 0, the [A | A2] seam inside a batch, the atomic split with a ragged last split
     and with a split that owns NO chunks; tile 7 (transposed store, bias by row); gemm_skinny_nn64_kernel at batch <2>
     and <4>, MT = 1 and 2, K < 64, an empty last split;
  C  the register-direct kernel (tile 9): NT (PIPE 0, BATCH 2) and NN (PIPE 1, BATCH 1), 4 and 8 waves, fewer chunks
     than waves, K odd, M = 31 / 33, N = 63 / 65, the [A | A2] seam inside a BATCH 2 pair, the five outcomes of
     pick_xcd_grid;
  D  the register-direct weight gradient (tile 10): overwrite and accumulate, K = 1, 15, 17, 333, split-K atomics, row
     strides wider than the matrix, an empty last split, and every accumulating row called twice into the same C:
     C0 + g, then C0 + 2 g;
  E  the k-contiguous LDS tiles 12-17 ragged around BM / BN at K = 32, 64, 96 with the A2 seam, accumulate and the
     XCD grids; tile 11 at its two thresholds and one step under each; ops.gemm_split; the grouped grid with an int
     twin of the mixed bag of test_grouped_weight_gradients_equal_the_single_launches and the edges of
     gemm_group.takes, read from the profile keys;
  F  ops.gemm with tile = -1: each routing branch once, result and profile keys;
  G  dv3_gemm_f32 with tile = -1 through ctypes (pick_tile, legacy_tile, the t == 9 fall-back under transA, the
     K1 % 64 fall-back), and the rejections that return DV3_ERR_ARG before a launch;
  H  a CPU self-check: a pure-Python COPY of the host arithmetic of gemm.hip (dv3_gemm_f32, launch_ts, launch_skinny,
     launch_skinny_nn64, launch_direct, launch_direct_tn, launch_l16, pick_xcd_grid) and of the tail of ops.gemm maps
     every row of A-G to a label (kernel, template arguments, split count, last / empty splits, batch depth, XCD grid,
     n_full / tail).  Each row lands where its table says, each property claimed above holds for the row that claims
     it, the labels together are every kernel instantiation the shipped library can reach, and ops.pick_gemm_tile
     agrees with the copied pick_tile on every y = x W^T row of F.  THE COPY MUST BE UPDATED TOGETHER WITH THE
     THRESHOLDS IN csrc/gemm.hip AND dv3hip/ops.py.

Three things the guards make unreachable, found while copying them (the rows use the nearest reachable call instead):
  * dv3_gemm_f32 rejects every A2 with K1 % 32 != 0, so no A2 call reaches the few-row or register-direct kernels with
    K1 = 16, and its `A2 && K1 % 16 != 0` fall-back lines never fire.  ops.gemm turns such a call into two launches
    (row "two-pass" of C and F).  The seam inside a BATCH 2 pair is reached with K1 = 96 instead (wave 1 starts at
    chunk 5, its pair (5, 6) straddles k = 96), the seam inside a few-row batch likewise;
  * with tile = -1, `t == 9 -> 6` needs M N > 512 k, which pick_tile's own t64 <= 128 excludes: it is reached only
    through legacy_tile after l16_ok fails (a TN call of mid size);
  * the K1 % 64 fall-back to tile 1 needs t in (5, 6, 8) next to an A2, which tile = -1 never gives (A2 forbids
    transA): it is reached with a forced tile 5 / 6 / 8 and K1 = 32, through ctypes.

Out of scope (development switches; DV3_ENV_INT / _dev.value are constants unless the library is built with
build.py --dev): DV3_DIRECT_* (RN 2 / 8, other batch depths, PIPE), DV3_L16_* (serial loop, serial epilogue, PF 2),
DV3_GROUP_TILE, DV3_XCD_M, DV3_SMALL_TILE / DV3_MID_TILE, DV3_BT_MIN_FLOPS.  Also: K = 0, lane tile choices.
Covered elsewhere: the scan epilogues (scan_*_gemm) in tests/test_ln_gru_f64_gpu.py, gemm_sample (EPI 1, ALN 1, its
[A | A2] seam) in tests/test_fused_f64_gpu.py, ens_gemm in tests/test_ens_f64_gpu.py.

Bars: 1e-4 * max(1, max |ref|) (TOL of tests/test_kernels_gpu.py, check() of tests/test_row_kernels_f64_gpu.py) for
every float comparison.  No bar here is widened: on every case below the fp32 CPU oracle's own error against float64
stays under half the bar (oracle_ratio() over every row, at dt=float32; asserted on the CPU by
test_fp32_oracle_error_is_under_half_the_bar).  Worst measured oracle error / bar per group:
  A 0.0054 (tile 6 NT 31x65x131), B 0.0053 (tile 3 NT 5x48x1281), C 0.0048 (tile 9 NN 31x65x496),
  D 0.0066 (tile 10 33x65x333), E 0.0041 (gemm_split, nsplit 48), F 0.0050 (NN 2048x1024x1696, odd lda),
  G 0.0033 (NT 640x1024x(32+32), odd lda).

Outcome: every row passed as written on an MI355X, the int runs bit-exact; no kernel or dispatch change was needed.
"""
import math

import pytest
import torch

from tests.test_row_kernels_f64_gpu import check, dev, gen

TOL = 1e-4
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
KINDS = ["randn", "int"]
PAD = 7777.0
ERR_ARG = 10001  # DV3_ERR_ARG of include/dv3hip.h (dv3hip/_lib.py check())
ORIENT = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}


@pytest.fixture(scope="module")
def ops():
    from dv3hip import ops as _ops

    return _ops


def cdiv(a, b):
    return -(-a // b)


def G(tile, o, M, N, K1, K2=0, bias=0, acc=False, win=False, lay="plain", twice=False, **claims):
    """One product.  acc: False | True | "atomic".  claims: what the row says about its launch, checked in H."""
    return dict(tile=tile, o=o, M=M, N=N, K1=K1, K2=K2, bias=bool(bias), acc=acc, win=bool(win), lay=lay, twice=twice,
                claims=claims)


def case_id(c):
    acc = {False: "", True: "+acc", "atomic": "+atomic"}[c["acc"]]
    return (f"t{c['tile']}-{c['o']}-{c['M']}x{c['N']}x{c['K1']}" + (f"+{c['K2']}" if c["K2"] else "") + acc +
            ("+bias" if c["bias"] else "") + ("+win" if c["win"] else "") + ("" if c["lay"] == "plain" else "+" + c["lay"]))


# ================================================================== H: the host arithmetic, copied from csrc/gemm.hip
# tile code -> (BM, BN, BK, WK) of the k-major LDS engine (the TileShape aliases above dv3_gemm_f32)
TS = {0: (128, 128, 16, 1), 1: (64, 64, 32, 1), 2: (32, 128, 32, 1), 4: (128, 128, 32, 1), 5: (64, 64, 64, 1),
      6: (32, 64, 64, 2), 8: (32, 32, 64, 4)}
L16 = {12: (64, 96), 13: (64, 64), 14: (32, 64), 15: (128, 128), 16: (128, 64), 17: (64, 128)}


def c_legacy_tile(M, N):
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if t64 <= 512:
        return 9
    c128 = cdiv(cdiv(M, 128) * cdiv(N, 128), 256) * 4
    c64 = cdiv(t64, 256)
    return 1 if c64 < c128 else 4


def c_pick_tile(M, N, K, acc):
    if M <= 32:
        return 2
    if acc and K >= 4096 and M * N >= 512 * 1024:
        return 4
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if t64 <= 128:
        return 9
    if cdiv(M, 128) * cdiv(N, 128) >= 448:
        return 15
    if t64 < 512:
        return 14
    if t64 <= 1024:
        return 13
    if t64 <= 2048 and (N >= 3072 or N <= 512):
        return 14
    return c_legacy_tile(M, N)


def c_xcd_grid(M, N, K, tiles_m, tiles_n):
    """pick_xcd_grid -> "8x1" | "4x2" | "2x4" | "1x8" | "linear"."""
    best, pick = 0.0, None
    for xm in (8, 4, 2, 1):
        xn = 8 // xm
        if tiles_m % xm or tiles_n % xn:
            continue
        cost = float(M) * K * xn + float(N) * K * xm
        if pick is None or cost < best:
            best, pick = cost, f"{xm}x{xn}"
    return pick or "linear"


def c_wave_walk(cb_ce, batch, K, K1):
    """The batch loop of the few-row / register-direct kernels over the (cb, ce) chunk ranges of the waves -> the load
    paths taken: "fast", "clamped" (a fast batch reaching past ce: its surplus chunks are clamped onto the last one),
    "tail" (slow: the batch runs past K), "seam" (slow although inside K: the A2 seam sits inside the batch)."""
    seen = set()
    for cb, ce in cb_ce:
        for c0 in range(cb, ce, batch):
            cend = min(c0 + batch, ce)
            if cend * 16 > K:
                seen.add("tail")
            elif not (c0 * 16 >= K1 or cend * 16 <= K1):
                seen.add("seam")
            else:
                seen.add("clamped" if c0 + batch > ce else "fast")
    return seen


def c_split_ranges(chunks, splits, waves):
    """Chunk ranges of the kernels that split K over gridDim.y workgroups, then over the waves -> (chunks owned by each
    workgroup, [(cb, ce) of every wave])."""
    per_wg = cdiv(chunks, splits)
    owned, ranges = [], []
    for y in range(splits):
        wcb, wce = y * per_wg, min(chunks, y * per_wg + per_wg)
        owned.append(max(wce - wcb, 0))
        per = cdiv(max(wce - wcb, 0), waves)
        for w in range(waves):
            cb = wcb + w * per
            ranges.append((cb, min(wce, cb + per)))
    return owned, ranges


def c_launch_ts(tile, o, M, N, K, hasA2, acc):
    BM, BN, BK, WK = TS[tile]
    tiles = cdiv(M, BM) * cdiv(N, BN)
    splits, chunk = 1, K
    if acc and not hasA2 and tiles < 192 and K >= 8 * BK:
        want = min(cdiv(384, tiles), K // (4 * BK))
        if want > 1:
            chunk = cdiv(cdiv(K, want), BK) * BK
            splits = cdiv(K, chunk)
    last = K - (splits - 1) * chunk
    return dict(inst=f"gemm_kernel<{tile},{o}>", tiles=tiles, splits=splits, chunk=chunk, last=last, wgs=tiles * splits,
                n_full=last // BK, tail=last % BK, WK=WK, atomics=splits > 1)


def c_launch_skinny(tb, MT, N, K, K1, acc):
    """N: the column count of the launch (tile 7: the rows of the call)."""
    tiles, chunks = cdiv(N, 16), cdiv(K, 16)
    splits, waves = 1, 8
    if acc == 2:
        waves = 4
        splits = min(cdiv(1024, tiles * waves), chunks // (2 * waves))
        if splits <= 1:
            splits, waves = 1, 8
    per = cdiv(cdiv(chunks, splits), waves)
    batch = 3 if per <= 3 else 6 if (per <= 6 or MT > 1) else 12
    owned, ranges = c_split_ranges(chunks, splits, waves)
    return dict(inst=f"skinny<{'T' if tb else 'N'},{MT},{batch}>", splits=splits, waves=waves, batch=batch, chunks=chunks,
                owned=owned, empty=sum(1 for v in owned if v == 0), paths=c_wave_walk(ranges, batch, K, K1),
                atomics=splits > 1)


def c_launch_nn64(MT, N, K):
    tiles, chunks = N // 64, cdiv(K, 16)
    splits = min(cdiv(256, tiles), max(chunks // 4, 1))
    per = cdiv(cdiv(chunks, splits), 4)
    batch = 2 if per <= 2 else 4
    owned, ranges = c_split_ranges(chunks, splits, 4)
    return dict(inst=f"nn64<{MT},{batch}>", splits=splits, batch=batch, per=per, chunks=chunks, owned=owned,
                empty=sum(1 for v in owned if v == 0), paths=c_wave_walk(ranges, batch, K, K), atomics=True)


def c_launch_direct(tb, M, N, K, K1):
    chunks = cdiv(K, 16)
    waves = 8 if chunks >= 32 else 4
    per = cdiv(chunks, waves)
    ranges = [(w * per, min(chunks, w * per + per)) for w in range(waves)]
    batch = 2 if tb else 1
    return dict(inst=f"direct<{'T' if tb else 'N'}>", waves=waves, chunks=chunks, batch=batch,
                xcd=c_xcd_grid(M, N, K, cdiv(M, 32), cdiv(N, 64)), paths=c_wave_walk(ranges, batch, K, K1))


def c_launch_direct_tn(M, N, K, acc):
    tiles, chunks = cdiv(M, 32) * cdiv(N, 64), cdiv(K, 16)
    splits = 1
    if acc:
        splits = max(1, min(cdiv(1024, tiles), chunks // 16))
    owned, _ = c_split_ranges(chunks, splits, 4)
    return dict(inst="direct_tn", splits=splits, chunks=chunks, owned=owned, empty=sum(1 for v in owned if v == 0),
                atomics=splits > 1)


def c_launch_l16(force, M, N, K):
    wgs = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)
    sel = 4 if wgs(128, 128) >= 448 else 2 if wgs(64, 64) >= 512 else 3
    if 1 <= force <= 6:
        sel = force
    bm = 32 if sel == 3 else 128 if sel in (4, 5) else 64
    bn = 96 if sel == 1 else 128 if sel in (4, 6) else 64
    return dict(inst=f"l16<{bm}x{bn}>", xcd=c_xcd_grid(M, N, K, cdiv(M, bm), cdiv(N, bn)), tiles=wgs(bm, bn))


def c_dispatch(ta, tb, M, N, K, K1, hasA2, bias, acc, tile, l16ok):
    """dv3_gemm_f32 -> the label of its launch, or "ERR_ARG".  acc: 0 | 1 | 2; l16ok: l16_ok() of the operands."""
    o = {(0, 1): "NT", (0, 0): "NN", (1, 0): "TN", (1, 1): "TT"}[(ta, tb)]
    if tile == 7:
        if ta or not tb or hasA2 or N > 32:
            return "ERR_ARG"
        return dict(c_launch_skinny(True, 1 if N <= 16 else 2, M, K, K, acc), tile=7)
    if not hasA2:
        K1 = K
    elif ta or K1 <= 0 or K1 >= K or K1 % 32:
        return "ERR_ARG"
    t = tile if (0 <= tile <= 6 or 8 <= tile <= 17) else c_pick_tile(M, N, K, acc)
    if t >= 11 and tile < 0 and not l16ok:
        t = c_legacy_tile(M, N)
    if t == 9 and tile < 0 and (ta or (hasA2 and K1 % 16)):
        t = 8 if M * N <= 512 * 1024 else 6
    if hasA2 and K1 % 64 and t in (5, 6, 8):
        t = 1
    if t == 3:
        if M > 128 or ta or (hasA2 and K1 % 16):
            return "ERR_ARG"
        if M <= 32 and acc == 2 and not tb and not hasA2 and N % 64 == 0:
            return dict(c_launch_nn64(1 if M <= 16 else 2, N, K), tile=3)
        return dict(c_launch_skinny(bool(tb), 1 if M <= 16 else 2, N, K, K1, acc), tile=3)
    if t == 10:
        if not ta or tb or hasA2 or bias:
            return "ERR_ARG"
        return dict(c_launch_direct_tn(M, N, K, acc), tile=10)
    if t >= 11:
        if not l16ok:
            return "ERR_ARG"
        return dict(c_launch_l16(t - 11, M, N, K), tile=t)
    if t == 9:
        if ta or (hasA2 and K1 % 16):
            return "ERR_ARG"
        return dict(c_launch_direct(bool(tb), M, N, K, K1), tile=9)
    return dict(c_launch_ts(t, o, M, N, K, hasA2, acc), tile=t)


# every kernel instantiation the shipped library reaches from dv3_gemm_f32, dv3_gemm_split_f32 and
# dv3_gemm_tn_grouped_f32 (the EPI / ALN forms belong to dv3_gemm_sample_f32: tests/test_fused_f64_gpu.py)
REACHABLE = ({f"gemm_kernel<{t},{o}>" for t in TS for o in ORIENT} |
             {f"skinny<{tb},{mt},{b}>" for tb in "TN" for mt, bs in ((1, (3, 6, 12)), (2, (3, 6))) for b in bs} |
             {f"nn64<{mt},{b}>" for mt in (1, 2) for b in (2, 4)} | {"direct<T>", "direct<N>", "direct_tn", "grouped"} |
             {f"l16<{bm}x{bn}>" for bm, bn in L16.values()})

# ---- the Python side: dv3hip/ops.py.  _TILE_NAMES, pick_gemm_tile, _legacy_tile and the tail of ops.gemm, copied
TILE_NAMES = {0: "128x128x16", 1: "64x64x32", 2: "32x128x32", 3: "skinny16", 4: "128x128x32", 5: "64x64x64",
              6: "32x64x64s2", 7: "narrowN", 8: "32x32x64s4", 9: "direct32x64", 10: "directTN32x64", 11: "l16",
              12: "l16_64x96", 13: "l16_64x64", 14: "l16_32x64", 15: "l16_128x128", 16: "l16_128x64", 17: "l16_64x128"}
BT_MIN_FLOPS = 7e9


def py_legacy_tile(M, N):
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if t64 <= 512:
        return 9
    c128 = cdiv(cdiv(M, 128) * cdiv(N, 128), 256) * 4
    return 1 if cdiv(t64, 256) < c128 else 4


def py_pick_gemm_tile(M, N, wgrad=False, K=0):
    if M <= 32:
        return 2
    if wgrad:
        return 4 if (K >= 4096 and M * N >= 512 * 1024) else 10
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if t64 <= 128:
        return 9
    if cdiv(M, 128) * cdiv(N, 128) >= 448:
        return 15
    if t64 < 512:
        return 14
    if t64 <= 1024:
        return 13
    if t64 <= 2048 and (N >= 3072 or N <= 512):
        return 14
    return py_legacy_tile(M, N)


def l16_auto_name(M, N):
    wgs = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)
    return "l16_128x128" if wgs(128, 128) >= 448 else "l16_64x64" if wgs(64, 64) >= 512 else "l16_32x64"


def lay_ok16(lay, cols):
    """Does a stored operand of `cols` columns in this layout meet l16_ok (ld % 4 == 0, base % 16 == 0)?"""
    return lay == "wide4" or (lay == "plain" and cols % 4 == 0)


def py_route(c):
    """ops.gemm on case c, outside a gemm_group -> [(profile key, label of the launch)] in launch order."""
    ta, tb = ORIENT[c["o"]]
    M, N, K1, K2 = c["M"], c["N"], c["K1"], c["K2"]
    acc = {False: 0, True: 1, "atomic": 2}[c["acc"]]

    def one(K1, K2, bias, acc, tile, b_off=0):
        K = K1 + K2
        hasA2 = K2 > 0
        # l16_ok of the operands as place() lays them out (b_off: B sliced b_off columns in, the two-pass path)
        ok = (not ta and tb and K >= 32 and K % 32 == 0 and K1 % 32 == 0 and lay_ok16(c["lay"], K1) and
              (not hasA2 or lay_ok16(c["lay"], K2)) and lay_ok16(c["lay"], K + b_off) and b_off % 4 == 0)
        if hasA2 and K1 % (64 if tile in (5, 6, 8) else 32):
            return one(K1, 0, bias, acc, tile) + one(K2, 0, False, acc or 1, tile, b_off=K1)
        if (tile < 0 and not ta and not tb and not hasA2 and 2.0 * M * N * K >= BT_MIN_FLOPS and
                py_pick_gemm_tile(M, N, False, K) >= 11 and K % 32 == 0 and lay_ok16(c["lay"], K)):
            t = py_pick_gemm_tile(M, N, False, K)  # (the scratch is contiguous and aligned: the l16 tile is taken)
            return [("dv3_transpose2d", None),
                    (f"gemm_kernel<{TILE_NAMES[t]},tA=0,tB=1>", c_dispatch(0, 1, M, N, K, K, False, bias, acc, t, True))]
        if tile < 0:
            tile = py_pick_gemm_tile(M, N, bool(ta), K)
            if M <= 32 and not ta:
                tile = 3
            if 32 < M <= 128 and tile == 9 and not ta and (not hasA2 or K1 % 16 == 0):
                tile = 3
            if tile in (6, 8) and hasA2 and K1 % 64:
                tile = 1
            if tile >= 11 and not ok:
                tile = py_legacy_tile(M, N)
            if tile == 9 and (ta or (hasA2 and K1 % 16)):
                tile = (8 if M * N <= 512 * 1024 else 6) if not (hasA2 and K1 % 64) else 1
            if tile == 10 and (tb or hasA2 or bias):
                tile = 1
            if N <= 32 and M > 32 and not ta and tb and not hasA2:
                tile = 7
        name = l16_auto_name(M, N) if tile == 11 else TILE_NAMES[tile]
        return [(f"gemm_kernel<{name},tA={ta},tB={tb}>", c_dispatch(ta, tb, M, N, K, K1, hasA2, bias, acc, tile, ok))]

    return one(K1, K2, c["bias"], acc, c["tile"])


def label(c):
    """The label of the (last) launch of case c through ops.gemm."""
    return py_route(c)[-1][1]


# ================================================================================================== the case tables
LAYS = ["plain", "odd", "off1"]


def engine_cases(tile, o):
    """Group A rows of one tile and orientation."""
    BM, BN, BK, _ = TS[tile]
    out = []
    shapes = [(BM - 1, BN + 1), (BM + 1, BN - 1), (BM + 1, BN + 1)]
    for j, K in enumerate([3, BK - 1, BK, BK + 1, 2 * BK + 3]):
        for s, (M, N) in enumerate(shapes):
            i = 3 * j + s
            out.append(G(tile, o, M, N, K, bias=i % 2, acc=bool((i // 2) % 2), win=(i % 4 == 1), lay=LAYS[(i + j) % 3]))
    if o in ("NT", "NN"):
        K1 = 64 if tile in (5, 6, 8) else 32
        for i, K2 in enumerate([1, 3, BK, BK + 5]):
            out.append(G(tile, o, BM + 1, BN + 1, K1, K2, bias=i % 2, acc=bool(i // 2), lay=LAYS[i % 3]))
    if o != "TT":
        # split-K of launch_ts: 4 tiles x 2 splits = 8 workgroups, 6 tiles x 2 = 12 (xcd_remap with a remainder)
        Ks = {0: 129, 1: 300, 8: 515}.get(tile, 8 * BK + 3)
        out.append(G(tile, o, BM + 1, BN + 1, Ks, bias=1, acc=True, splits=2, wgs=8))
        out.append(G(tile, o, 2 * BM + 1, BN + 1, Ks, bias=1, acc=True, lay="odd", splits=2, wgs=12))
        if tile == 1:
            out.append(G(tile, o, BM + 1, BN + 1, 1000, bias=1, acc=True, win=True, splits=7, wgs=28))
        if tile in (6, 8):  # the wave-group reduce under accumulate WITHOUT workgroup split-K (K < 8 BK)
            out.append(G(tile, o, BM + 1, BN + 1, 7 * BK + 1, bias=1, acc=True, splits=1))
    return out


ENGINE_TILES = [0, 1, 2, 4, 5, 6, 8]
ENGINE = {(t, o): engine_cases(t, o) for t in ENGINE_TILES for o in ORIENT}

# B: tile 3.  batch: the register batch depth <3> / <6> / <12>; paths: load paths that must occur (c_wave_walk)
SKINNY_ROWS = [
    G(3, "NT", 1, 1, 17, bias=1, batch=3, fewer_chunks_than_waves=True, paths={"tail"}),   # K % 16, K % 4 != 0
    G(3, "NN", 15, 15, 384, acc=True, batch=3, paths={"fast"}),                            # per = 3 exactly
    G(3, "NT", 16, 17, 385, bias=1, acc="atomic", lay="odd", batch=3, splits=3),           # 25 chunks: 9 + 9 + 7
    G(3, "NT", 16, 300, 768, bias=1, batch=6, paths={"fast"}),                             # per = 6 exactly
    G(3, "NT", 16, 48, 800, win=True, batch=12, paths={"clamped"}),                        # per = 7 in a batch of 12
    G(3, "NN", 1, 17, 1000, bias=1, acc=True, batch=12, paths={"clamped", "tail"}),        # K % 16 != 0, MT = 1
    G(3, "NT", 17, 15, 770, acc=True, lay="off1", batch=6, paths={"clamped", "tail"}),     # MT = 2: <6> although per = 7
    G(3, "NN", 31, 300, 50, bias=1, batch=3, fewer_chunks_than_waves=True, paths={"tail"}),  # K % 4 != 0
    G(3, "NT", 32, 17, 500, acc="atomic", bias=1, batch=3, splits=4),                    # 32 chunks as 8 x 4
    G(3, "NN", 33, 15, 100, win=True, lay="odd", batch=3),                                 # grid.z = 2, one row in the second
    G(3, "NT", 48, 300, 64, 37, acc=True, bias=1, batch=3, paths={"clamped", "tail"}),     # A2, K2 ragged
    G(3, "NN", 127, 17, 32, 5, acc="atomic", bias=1, batch=3, splits=1),
    G(3, "NT", 128, 1, 400, bias=1, batch=6),
    G(3, "NN", 128, 300, 96, acc=True, batch=3),
    G(3, "NT", 16, 17, 96, 300, bias=1, batch=6, paths={"seam"}),                          # the seam inside a batch of 6
    G(3, "NN", 16, 15, 96, 700, acc=True, batch=12, paths={"seam"}),                       # ... and of 12
    G(3, "NT", 32, 15, 32, 3, lay="odd", batch=3),
    G(3, "NN", 15, 17, 700, bias=1, lay="odd", batch=6, inst="skinny<N,1,6>"),
    G(3, "NN", 48, 15, 1000, acc=True, win=True, batch=6, inst="skinny<N,2,6>"),
    G(3, "NN", 15, 300, 600, acc="atomic", bias=1, batch=3),                               # N % 64 != 0: not nn64
    # the atomic split: 33 chunks as 9 + 9 + 9 + 6
    G(3, "NT", 7, 33, 520, acc="atomic", bias=1, batch=3, splits=4, owned=[9, 9, 9, 6]),
    # 81 chunks over 10 splits of 9: workgroup 9 owns none (K = 1281 .. 1296)
    G(3, "NT", 5, 48, 1281, acc="atomic", bias=1, splits=10, empty=1),
    G(3, "NN", 9, 48, 1296, acc="atomic", bias=1, splits=10, empty=1),
    G(3, "NT", 20, 48, 1290, acc="atomic", bias=1, win=True, splits=10, empty=1),          # MT = 2
]
# tile 7: C^T = W A^T on the few-row kernel (the call's N <= 32 are its rows), transposed store, bias by row
NARROW_ROWS = [
    G(7, "NT", 33, 1, 17, bias=1, batch=3),
    G(7, "NT", 100, 6, 100, bias=1, acc=True, win=True, batch=3),
    G(7, "NT", 33, 16, 800, bias=1, acc="atomic", batch=3, splits=6),
    G(7, "NT", 100, 17, 400, acc=False, win=True, lay="odd", batch=6),
    G(7, "NT", 33, 32, 1000, bias=1, acc=True, batch=6),                                   # MT = 2
    G(7, "NT", 100, 1, 900, acc=True, bias=1, batch=12),
    G(7, "NT", 33, 6, 50, acc="atomic", win=True, batch=3, splits=1),
    G(7, "NT", 100, 16, 64, lay="off1", bias=1, batch=3),
    G(7, "NT", 100, 32, 2600, acc="atomic", bias=1, win=True, splits=20),
    G(7, "NT", 33, 17, 3, acc=True, bias=1, batch=3),
]
# gemm_skinny_nn64_kernel: M <= 32, "atomic", B as [K][N], N % 64 == 0, no A2
NN64_ROWS = [
    G(3, "NN", 16, 4096, 758, acc="atomic", bias=1, inst="nn64<1,4>", splits=4, paths={"clamped", "tail"}),  # per = 3
    G(3, "NN", 32, 4096, 758, acc="atomic", inst="nn64<2,4>", splits=4),
    G(3, "NN", 8, 64, 40, acc="atomic", bias=1, inst="nn64<1,2>", splits=1),               # K < 64: one split, atomics
    G(3, "NN", 1, 192, 64, acc="atomic", inst="nn64<1,2>", lay="odd", splits=1),
    G(3, "NN", 17, 64, 300, acc="atomic", bias=1, win=True, inst="nn64<2,2>"),
    # 25 chunks over 6 splits of 5: workgroup 5 owns none (K = 385 .. 400)
    G(3, "NN", 32, 128, 385, acc="atomic", bias=1, inst="nn64<2,2>", splits=6, empty=1),
    G(3, "NN", 16, 128, 400, acc="atomic", bias=1, inst="nn64<1,2>", splits=6, empty=1),
]
# C: tile 9
DIRECT_ROWS = [G(9, o, M, N, K1, K2, bias=b, acc=a, win=w, lay=l, **cl) for o in ("NT", "NN") for
               (M, N, K1, K2, b, a, w, l, cl) in [
    (31, 63, 17, 0, 1, False, 0, "plain", dict(waves=4, fewer_chunks_than_waves=True)),
    (33, 65, 37, 0, 0, True, 1, "odd", dict(waves=4)),                                     # K odd
    (33, 63, 499, 0, 1, True, 0, "off1", dict(waves=8)),                                   # 32 chunks: 8 waves, K odd
    (31, 65, 496, 0, 0, False, 0, "plain", dict(waves=4)),                                 # 31 chunks: still 4 waves
    (33, 65, 520, 0, 1, False, 1, "plain", dict(waves=8)),                                 # 33 chunks, 8 waves of 5: wave 7 idle
    (33, 65, 32, 5, 1, False, 0, "odd", dict(waves=4)),
    (33, 65, 96, 200, 1, True, 0, "plain", dict(waves=4, seam_in_pair=True)),              # wave 1: chunks 5 .. 9
    (33, 65, 16, 21, 1, True, 0, "plain", dict(two_pass=True)),                            # K1 = 16: ops.gemm splits it
    (256, 64, 32, 0, 1, False, 0, "plain", dict(xcd="8x1")),
    (128, 128, 32, 0, 0, True, 0, "plain", dict(xcd="4x2")),
    (64, 256, 32, 0, 1, False, 0, "plain", dict(xcd="2x4")),
    (96, 512, 32, 0, 0, False, 0, "plain", dict(xcd="1x8")),
    (96, 192, 32, 0, 1, True, 0, "plain", dict(xcd="linear")),
]]
# D: tile 10 (C[M,N] (+)= A^T B, A [K][M], B [K][N]); every accumulating row is called twice
TN_ROWS = [
    G(10, "TN", 33, 65, 1, splits=1),
    G(10, "TN", 31, 63, 15, acc=True, twice=True, lay="odd", splits=1),
    G(10, "TN", 33, 65, 17, win=True, splits=1),
    G(10, "TN", 70, 130, 333, acc=True, twice=True, win=True, lay="odd", splits=1),        # 21 chunks: no split yet
    G(10, "TN", 33, 65, 333, lay="off1", splits=1),
    G(10, "TN", 33, 65, 1000, acc=True, twice=True, lay="odd", splits=3),                  # 63 chunks as 21 x 3
    G(10, "TN", 40, 100, 1030, acc=True, twice=True, splits=4, owned=[17, 17, 17, 14]),    # ragged last split
    G(10, "TN", 32, 64, 1000, splits=1),                                                   # overwrite never splits
    # one 32 x 64 tile, 289 chunks over 18 splits of 17: workgroup 17 owns none (K = 4609 .. 4624)
    G(10, "TN", 32, 64, 4610, acc=True, twice=True, splits=18, empty=1),
    G(10, "TN", 30, 60, 4624, acc=True, twice=True, splits=18, empty=1),
]


def l16_cases(tile):
    bm, bn = L16[tile]
    rows = [G(tile, "NT", bm + 1, bn - 1, 32, bias=1), G(tile, "NT", bm - 1, bn + 1, 64, acc=True, win=True, lay="wide4"),
            G(tile, "NT", bm + 1, bn + 1, 96, bias=1, acc=True), G(tile, "NT", bm + 1, bn + 1, 32, 32, bias=1, lay="wide4"),
            G(tile, "NT", 2 * bm + 1, bn + 1, 64, 32, acc=True, win=True)]
    for (tm, tn), xcd in (((8, 1), "8x1"), ((4, 2), "4x2"), ((2, 4), "2x4"), ((3, 8), "1x8"), ((3, 3), "linear")):
        rows.append(G(tile, "NT", tm * bm, tn * bn - 3, 32, bias=tm % 2, acc=tn > 2, xcd=xcd))
    return rows


L16_CASES = {t: l16_cases(t) for t in L16}
# tile 11 picks its shape by size: 128 x 128 from 448 such tiles, 64 x 64 from 512 such tiles, else 32 x 64
AUTO_ROWS = [G(11, "NT", 3584, 2048, 32, bias=1, inst="l16<128x128>", tiles=448),
             G(11, "NT", 3456, 2048, 32, inst="l16<64x64>", tiles=1728),                   # 432 tiles of 128 x 128
             G(11, "NT", 2048, 1024, 32, acc=True, inst="l16<64x64>", tiles=512),
             G(11, "NT", 1984, 1024, 32, bias=1, inst="l16<32x64>", tiles=992)]            # 496 tiles of 64 x 64
SPLIT_NS = [16, 48, 64]             # nsplit: inside a wave's 32-column block (16, 48) and on a tile edge (64)
SPLIT_SHAPE = (70, 40, 64)          # M (ragged), the columns of C2, K -> the 32 x 64 tile
# the grouped grid: (M, N, K, grouped?) -- gemm_group.takes is 32 <= K <= 2048 and M > 32 and N > 32
GROUP_ROWS = [(255, 129, 64, True), (100, 70, 96, True), (64, 64, 37, True), (33, 1030, 40, True), (65, 33, 32, True),
              (33, 33, 31, False), (34, 35, 2048, True), (35, 34, 2049, False), (32, 40, 64, False), (40, 32, 64, False),
              (33, 33, 33, True)]

# F: ops.gemm with tile = -1.  keys: the profile keys of the call, in order (a pair: (key, launches))
K_ = lambda name, o: f"gemm_kernel<{name},tA={ORIENT[o][0]},tB={ORIENT[o][1]}>"
ROUTE_ROWS = [
    G(-1, "NT", 16, 100, 70, bias=1, keys=[K_("skinny16", "NT")], inst="skinny<T,1,3>"),               # M <= 32
    G(-1, "NN", 30, 100, 70, acc=True, keys=[K_("skinny16", "NN")], inst="skinny<N,2,3>"),
    G(-1, "NT", 100, 200, 50, bias=1, keys=[K_("skinny16", "NT")], inst="skinny<T,2,3>"),              # 32 < M <= 128
    G(-1, "NT", 200, 6, 64, bias=1, keys=[K_("narrowN", "NT")], inst="skinny<T,1,3>"),                 # N <= 32, M > 32
    G(-1, "NT", 200, 6, 32, 32, bias=1, keys=[K_("direct32x64", "NT")], inst="direct<T>"),             # ... not with A2
    G(-1, "TN", 6, 50, 100, acc=True, keys=[K_("32x128x32", "TN")], inst="gemm_kernel<2,TN>"),         # Nout = 6
    G(-1, "TN", 70, 50, 100, acc=True, keys=[K_("directTN32x64", "TN")], inst="direct_tn"),
    G(-1, "TN", 512, 1024, 4100, acc=True, keys=[K_("128x128x32", "TN")], inst="gemm_kernel<4,TN>", splits=12),
    G(-1, "NT", 640, 1024, 32, bias=1, keys=[K_("l16_32x64", "NT")], inst="l16<32x64>"),               # t64 = 160
    G(-1, "NT", 2048, 1024, 32, keys=[K_("l16_64x64", "NT")], inst="l16<64x64>"),                      # t64 = 512
    G(-1, "NT", 3584, 2048, 32, bias=1, keys=[K_("l16_128x128", "NT")], inst="l16<128x128>"),          # 448 tiles
    G(-1, "NT", 8320, 512, 32, keys=[K_("l16_32x64", "NT")], inst="l16<32x64>"),                       # tall: t64 = 1040
    G(-1, "NT", 2048, 2112, 32, keys=[K_("64x64x32", "NT")], inst="gemm_kernel<1,NT>"),                # pick_tile's last line
    # the fall-back from the k-contiguous LDS tiles: K % 32, lda % 4, a 4-byte-aligned base
    G(-1, "NT", 640, 1024, 40, bias=1, keys=[K_("direct32x64", "NT")], inst="direct<T>"),
    G(-1, "NT", 640, 1024, 32, lay="odd", keys=[K_("direct32x64", "NT")], inst="direct<T>"),
    G(-1, "NT", 640, 1024, 32, lay="off1", acc=True, keys=[K_("direct32x64", "NT")], inst="direct<T>"),
    G(-1, "NT", 2048, 1100, 40, keys=[K_("64x64x32", "NT")], inst="gemm_kernel<1,NT>"),
    G(-1, "NT", 4096, 2048, 40, bias=1, keys=[K_("128x128x32", "NT")], inst="gemm_kernel<4,NT>"),
    # A2 with K1 % 32 != 0: two launches, the bias in the first only
    G(-1, "NT", 70, 50, 20, 13, bias=1, keys=[(K_("skinny16", "NT"), 2)], two_pass=True),
    G(-1, "NT", 70, 50, 20, 13, bias=1, acc=True, keys=[(K_("skinny16", "NT"), 2)], two_pass=True),
    G(-1, "NN", 70, 50, 48, 13, bias=1, acc="atomic", keys=[(K_("skinny16", "NN"), 2)], two_pass=True),
    # NN above DV3_BT_MIN_FLOPS = 7e9 (2 x 2048 x 1024 x 1696 = 7.11e9): the transposed copy, then the 64 x 64 tile
    G(-1, "NN", 2048, 1024, 1696, bias=1, keys=["dv3_transpose2d", K_("l16_64x64", "NT")], inst="l16<64x64>"),
    G(-1, "NN", 2048, 1024, 1696, lay="odd", acc=True, keys=[K_("direct32x64", "NN")], inst="direct<N>"),  # odd lda: not taken
]
# G: dv3_gemm_f32 with tile = -1 through ctypes (rows that need no Python-side preparation), and two forced tiles
LIB_ROWS = [
    G(-1, "NT", 16, 100, 70, bias=1, inst="gemm_kernel<2,NT>"),                            # pick_tile: M <= 32
    G(-1, "NN", 30, 100, 70, acc=True, inst="gemm_kernel<2,NN>"),
    G(-1, "NT", 100, 200, 50, bias=1, inst="direct<T>"),                                   # t64 <= 128
    G(-1, "NN", 100, 200, 32, 18, acc=True, inst="direct<N>"),
    G(-1, "TN", 70, 50, 100, acc=True, inst="gemm_kernel<8,TN>"),                          # t == 9 under transA, M N <= 512 k
    G(-1, "TT", 70, 50, 100, bias=1, inst="gemm_kernel<8,TT>"),
    G(-1, "TN", 640, 1024, 32, acc=True, inst="gemm_kernel<6,TN>"),                        # 14 -> legacy 9 -> 6 (M N > 512 k)
    G(-1, "TN", 512, 1024, 4100, acc=True, inst="gemm_kernel<4,TN>", splits=12),           # long reduction, big output
    G(-1, "NT", 640, 1024, 32, bias=1, inst="l16<32x64>"),
    G(-1, "NT", 2048, 1024, 32, inst="l16<64x64>"),
    G(-1, "NT", 3584, 2048, 32, bias=1, inst="l16<128x128>"),
    G(-1, "NT", 8320, 512, 32, inst="l16<32x64>"),
    G(-1, "NT", 2048, 2112, 32, inst="gemm_kernel<1,NT>"),                                 # legacy_tile from pick_tile
    G(-1, "NT", 640, 1024, 40, bias=1, inst="direct<T>"),                                  # legacy_tile after l16_ok fails
    G(-1, "NT", 2048, 1100, 40, inst="gemm_kernel<1,NT>"),
    G(-1, "NT", 4096, 2048, 40, bias=1, inst="gemm_kernel<4,NT>"),
    G(-1, "NT", 640, 1024, 32, 32, lay="odd", inst="direct<T>"),
    G(5, "NT", 65, 65, 32, 7, bias=1, inst="gemm_kernel<1,NT>"),                           # K1 % 64 != 0: tile 1
    G(6, "NN", 33, 65, 32, 64, acc=True, inst="gemm_kernel<1,NN>"),
    G(8, "NT", 33, 33, 32, 5, inst="gemm_kernel<1,NT>"),
]
# rejections: DV3_ERR_ARG before any launch.  (what, tile, orientation, M, N, K1, K2, bias)
REJECT_ROWS = [("tile 7 with N > 32", 7, "NT", 40, 33, 32, 0, False), ("tile 3 with M > 128", 3, "NT", 129, 16, 32, 0, False),
               ("tile 10 with bias", 10, "TN", 40, 40, 32, 0, True), ("tile 14 with K % 32 != 0", 14, "NT", 40, 70, 40, 0, False),
               ("tile 11 with K % 32 != 0", 11, "NT", 40, 70, 33, 0, False), ("A2 with transA", 1, "TN", 40, 40, 32, 32, False),
               ("A2 with K1 % 32 != 0", 9, "NT", 40, 40, 16, 16, False)]

GROUPS = {
    "A": [c for cs in ENGINE.values() for c in cs],
    "B": SKINNY_ROWS + NARROW_ROWS + NN64_ROWS,
    "C": DIRECT_ROWS,
    "D": TN_ROWS,
    "E": [c for cs in L16_CASES.values() for c in cs] + AUTO_ROWS,
    "F": ROUTE_ROWS,
    "G": LIB_ROWS,
}

# Exactness of the integer runs is a property of the inputs: |a b| <= 9 per term, K terms, + prefill (3) + bias (3); a
# row called twice adds its product twice.  Integers below 2^23 are exact in fp32, in every order of summation.
MAX_K = max(max((c["K1"] + c["K2"]) * (2 if c["twice"] else 1) for cs in GROUPS.values() for c in cs),
            max(r[2] for r in GROUP_ROWS), SPLIT_SHAPE[2])
assert MAX_K == 2 * 4624 and 9 * MAX_K + 6 < 2 ** 23


# ========================================================================================================== H: checks
def test_every_row_lands_on_its_kernel_and_every_kernel_has_a_row():
    """H.  The functions above are a COPY of the host arithmetic of csrc/gemm.hip and of the tail of ops.gemm (shipped
    library: every development switch at its default); they must be updated together with the thresholds there."""
    seen = set()
    for grp, cases in GROUPS.items():
        for c in cases:
            route = py_route(c) if grp != "G" else None
            if grp == "G":
                ta, tb = ORIENT[c["o"]]
                K = c["K1"] + c["K2"]
                ok = (c["o"] == "NT" and K % 32 == 0 and c["K1"] % 32 == 0 and c["lay"] in ("plain", "wide4"))
                lab = c_dispatch(ta, tb, c["M"], c["N"], K, c["K1"], c["K2"] > 0, c["bias"],
                                 {False: 0, True: 1, "atomic": 2}[c["acc"]], c["tile"], ok)
                labs = [lab]
            else:
                labs = [l for _, l in route if l is not None]
            assert all(l != "ERR_ARG" for l in labs), (grp, case_id(c), "a row the guards reject")
            lab = labs[-1]
            seen.update(l["inst"] for l in labs)
            cl = dict(c["claims"])
            if "keys" in cl:
                want = [k if isinstance(k, tuple) else (k, 1) for k in cl.pop("keys")]
                got = {}
                for k, _ in route:
                    got[k] = got.get(k, 0) + 1
                assert list(got.items()) == want, (case_id(c), got, want)
            if cl.pop("two_pass", False):
                assert len(route) == 2 and route[0][1]["inst"] == route[1][1]["inst"], (case_id(c), route)
            if cl.pop("fewer_chunks_than_waves", False):
                assert lab["chunks"] < lab["waves"], (case_id(c), lab)
            if cl.pop("seam_in_pair", False):
                assert ("seam" in lab["paths"]) == (lab["batch"] == 2), (case_id(c), lab)
            for k, v in cl.items():
                if k == "paths":
                    assert v <= lab["paths"], (case_id(c), k, lab["paths"], v)
                else:
                    assert lab[k] == v, (case_id(c), k, lab[k], v)
            assert not (c["twice"] and c["bias"]), case_id(c)  # (a second call would add the bias again)
            if c["tile"] >= 0 and grp != "G":
                assert lab["tile"] == c["tile"], (case_id(c), lab)
            if lab.get("atomics"):
                assert c["acc"] in (True, "atomic"), (case_id(c), "atomics into an overwritten C")
    seen |= {"grouped"}
    assert seen == REACHABLE, sorted(seen ^ REACHABLE)

    # ---- A: what the engine rows must reach, per tile and orientation
    for (tile, o), cases in ENGINE.items():
        BM, BN, BK, WK = TS[tile]
        labs = [label(c) for c in cases]
        plain = [(c, l) for c, l in zip(cases, labs) if not c["K2"] and l["splits"] == 1]
        assert {(l["n_full"], l["tail"]) for _, l in plain} >= {(0, 3), (0, BK - 1), (1, 0), (1, 1), (2, 3)}
        for key, vals in (("bias", {False, True}), ("acc", {False, True}), ("win", {False, True}), ("lay", set(LAYS))):
            assert {c[key] for c in cases} == vals, (tile, o, key)
        assert any(c["M"] % BM == 1 and c["N"] % BN == 1 for c in cases)
        if o in ("NT", "NN"):
            assert {c["K2"] for c in cases if c["K2"]} == {1, 3, BK, BK + 5}
            assert all(c["K1"] % BK == 0 and c["K1"] % 32 == 0 for c in cases if c["K2"])
        if o != "TT":
            sp = [(c, l) for c, l in zip(cases, labs) if l["splits"] > 1]
            assert all(c["bias"] and c["acc"] is True and l["last"] % BK and l["last"] < l["chunk"] for c, l in sp)
            assert {l["wgs"] % 8 for _, l in sp} >= {0, 4}
            if WK > 1:
                assert any(c["acc"] is True and l["splits"] == 1 and c["K1"] > 2 * BK for c, l in zip(cases, labs))
    # the split arithmetic the issue quotes
    for tile, K, chunk, last in ((1, 300, 160, 140), (0, 129, 80, 49), (8, 515, 320, 195)):
        BM, BN = TS[tile][:2]
        lab = c_launch_ts(tile, "NT", BM + 1, BN + 1, K, False, 1)
        assert (lab["tiles"], lab["splits"], lab["chunk"], lab["last"]) == (4, 2, chunk, last), lab
    assert c_launch_ts(1, "NT", 65, 65, 1000, False, 1)["splits"] == 7

    # ---- B: the sets of M and N the issue lists, the accumulate modes in both layouts, the depths
    t3 = [c for c in SKINNY_ROWS]
    assert {c["M"] for c in t3} >= {1, 15, 16, 17, 31, 32, 33, 48, 127, 128} and {c["N"] for c in t3} >= {1, 15, 17, 300}
    assert {(c["o"], c["acc"]) for c in t3} == {(o, a) for o in ("NT", "NN") for a in (False, True, "atomic")}
    assert {c["N"] for c in NARROW_ROWS} == {1, 6, 16, 17, 32} and {c["M"] for c in NARROW_ROWS} == {33, 100}
    assert {c["acc"] for c in NARROW_ROWS} == {False, True, "atomic"} and any(c["win"] for c in NARROW_ROWS)
    for K in range(1281, 1297):
        lab = c_launch_skinny(True, 1, 48, K, K, 2)
        assert lab["splits"] == 10 and lab["owned"] == [9] * 9 + [0], (K, lab)
    for K in range(385, 401):
        lab = c_launch_nn64(2, 128, K)
        assert lab["splits"] == 6 and lab["owned"] == [5] * 5 + [0], (K, lab)
    lab = c_launch_nn64(1, 4096, 758)
    assert (lab["splits"], lab["per"], lab["batch"]) == (4, 3, 4)
    # ---- C: both wave counts in both layouts, every XCD grid
    for o in ("NT", "NN"):
        labs = [label(c) for c in DIRECT_ROWS if c["o"] == o]
        assert {l["waves"] for l in labs} == {4, 8} and {l["xcd"] for l in labs} >= {"8x1", "4x2", "2x4", "1x8", "linear"}
    assert c_launch_direct(True, 33, 65, 497, 497)["waves"] == 8 and c_launch_direct(True, 33, 65, 496, 496)["waves"] == 4
    # ---- D
    for K in range(4609, 4625):
        lab = c_launch_direct_tn(32, 64, K, 1)
        assert lab["splits"] == 18 and lab["owned"] == [17] * 17 + [0], (K, lab)
    assert {c["K1"] for c in TN_ROWS} >= {1, 15, 17, 333}
    assert all(c["twice"] == (c["acc"] is True) for c in TN_ROWS)
    # ---- E
    for tile, cases in L16_CASES.items():
        assert {label(c)["xcd"] for c in cases} >= {"8x1", "4x2", "2x4", "1x8", "linear"}, tile
        assert {c["K1"] + c["K2"] for c in cases} >= {32, 64, 96} and any(c["K2"] for c in cases)
    M, n2, K = SPLIT_SHAPE
    assert all(c_launch_l16(0, M, ns + n2, K)["inst"] == "l16<32x64>" for ns in SPLIT_NS)
    assert [ns % 32 for ns in SPLIT_NS] == [16, 16, 0] and SPLIT_NS[2] % 64 == 0
    for M, N, K, grouped in GROUP_ROWS:
        assert grouped == (32 <= K <= 2048 and M > 32 and N > 32), (M, N, K)
    assert {(K, g) for M, N, K, g in GROUP_ROWS} >= {(31, False), (32, True), (2048, True), (2049, False)}
    assert any(K % 32 for _, _, K, g in GROUP_ROWS if g)
    # ---- F: ops.pick_gemm_tile against the library's pick_tile on every y = x W^T row (M <= 32 differs by design: the
    # library takes the 32 x 128 LDS tile there, ops.gemm overrides its own 2 with the few-row kernel)
    from dv3hip import ops

    for c in ROUTE_ROWS:
        K = c["K1"] + c["K2"]
        assert ops.pick_gemm_tile(c["M"], c["N"], c["o"][0] == "T", K) == py_pick_gemm_tile(c["M"], c["N"], c["o"][0] == "T", K)
        if c["o"] == "NT":
            assert ops.pick_gemm_tile(c["M"], c["N"], False, K) == c_pick_tile(c["M"], c["N"], K, 0), case_id(c)
    assert ops._TILE_NAMES == TILE_NAMES and ops._BT_MIN_FLOPS == BT_MIN_FLOPS
    assert 2.0 * 2048 * 1024 * 1696 >= BT_MIN_FLOPS > 2.0 * 2048 * 1024 * 1664
    for what, tile, o, M, N, K1, K2, bias in REJECT_ROWS:
        ta, tb = ORIENT[o]
        assert c_dispatch(ta, tb, M, N, K1 + K2, K1, K2 > 0, bias, 0, tile, (K1 + K2) % 32 == 0 and o == "NT") == "ERR_ARG", what


# ====================================================================================================== the reference
def reference(A, A2, B, bias, C0, ta, tb, dt=F64, times=1):
    """C0 + times * cat([A^T if ta else A, A2], -1) @ (B^T if tb else B) + bias, evaluated in dt on the CPU."""
    a = A.to(dt).t() if ta else A.to(dt)
    if A2 is not None:
        a = torch.cat([a, A2.to(dt)], -1)
    b = B.to(dt).t() if tb else B.to(dt)
    r = a @ b
    if times != 1:
        r = r * times
    if bias is not None:
        r = r + bias.to(dt)
    if C0 is not None:
        r = r + C0.to(dt)
    return r


def seed_of(c, kind):
    s = sum(ord(ch) for ch in c["o"] + c["lay"]) + (977 if kind == "int" else 0) + 31 * (c["tile"] + 2)
    for v in (c["M"], c["N"], c["K1"], c["K2"], int(c["bias"]), {False: 0, True: 1, "atomic": 2}[c["acc"]]):
        s = (s * 1009 + int(v)) % (2 ** 31 - 1)
    return s


def draw(shape, kind, g, scale=1.0):
    if kind == "int":
        return torch.randint(-3, 4, tuple(shape), generator=g).to(F32)
    return torch.randn(*shape, generator=g) * scale


def operands(c, kind):
    """-> (A, A2, B, bias, C0) on the CPU, as the kernel is given them (A as [K1][M] under transA, ...)."""
    ta, tb = ORIENT[c["o"]]
    M, N, K1, K2 = c["M"], c["N"], c["K1"], c["K2"]
    K = K1 + K2
    g = gen(seed_of(c, kind))
    sa, sb = (1.0 / math.sqrt(K), 1.0) if ta else (1.0, 1.0 / math.sqrt(K))
    A = draw((K1, M) if ta else (M, K1), kind, g, sa)
    A2 = draw((M, K2), kind, g, sa) if K2 else None
    B = draw((N, K) if tb else (K, N), kind, g, sb)
    bias = draw((N,), kind, g) if c["bias"] else None
    C0 = draw((M, N), kind, g) if c["acc"] else None
    return A, A2, B, bias, C0


def oracle_ratio(c):
    """The fp32 CPU oracle's own error against float64 on the randn operands of c, as a fraction of the bar."""
    ta, tb = ORIENT[c["o"]]
    A, A2, B, bias, C0 = operands(c, "randn")
    times = 2 if c["twice"] else 1
    r64 = reference(A, A2, B, bias, C0, ta, tb, F64, times)
    r32 = reference(A, A2, B, bias, C0, ta, tb, F32, times)
    return (r32.double() - r64).abs().max().item() / (TOL * max(1.0, r64.abs().max().item()))


def split_operands(nsplit, kind):
    """-> (generator, A [M, K], W [nsplit + n2, K]) of the gemm_split cases."""
    M, n2, K = SPLIT_SHAPE
    g = gen(4000 + nsplit + (977 if kind == "int" else 0))
    return g, draw((M, K), kind, g), draw((nsplit + n2, K), kind, g, 1.0 / math.sqrt(K))


def group_operands(kind):
    """-> [(A [K, M], B [K, N], C0 [M, N])] of GROUP_ROWS."""
    g = gen(5000 + (977 if kind == "int" else 0))
    return [(draw((K, M), kind, g, 1.0 / math.sqrt(K)), draw((K, N), kind, g), draw((M, N), kind, g))
            for M, N, K, _ in GROUP_ROWS]


def test_fp32_oracle_error_is_under_half_the_bar():
    """The bar is not widened anywhere: on the randn operands of every row the same reference evaluated in fp32 on the
    CPU stays under half of 1e-4 * max(1, max |ref|) from the float64 one (the worst ratios are in the module
    docstring).  CPU only; no kernel is involved."""
    worst = {}
    for grp, cases in GROUPS.items():
        for c in cases:
            worst[grp] = max(worst.get(grp, 0.0), oracle_ratio(c))
    for nsplit in SPLIT_NS:
        _, A, W = split_operands(nsplit, "randn")
        r64 = A.double() @ W.double().t()
        worst["E"] = max(worst["E"], ((A @ W.t()).double() - r64).abs().max().item() / (TOL * max(1.0, r64.abs().max().item())))
    for a, b, c0 in group_operands("randn"):
        r64 = c0.double() + a.double().t() @ b.double()
        worst["E"] = max(worst["E"], ((c0 + a.t() @ b).double() - r64).abs().max().item() / (TOL * max(1.0, r64.abs().max().item())))
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v < 0.5 for v in worst.values()), worst


# ============================================================================================================ helpers
def place(t, lay):
    """A GPU copy of the 2-D tensor t in layout lay; padding columns hold PAD."""
    if t is None:
        return None
    R, Cn = t.shape
    if lay == "plain":
        return dev(t)
    if lay == "off1":
        buf = torch.full((R * Cn + 8,), PAD, device="cuda")
        v = buf[1:1 + R * Cn].view(R, Cn)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    ld = Cn + 8 if lay == "wide4" else Cn + 5 + (Cn % 2)  # "odd": an odd leading dimension
    assert lay == "wide4" or ld % 2 == 1
    buf = torch.full((R, ld), PAD, device="cuda")
    v = buf[:, :Cn]
    v.copy_(t)
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


class Out:
    """The output C of a case: NaN (overwrite) or the seeded prefill (accumulate), alone or as the window
    [:, 3 : 3 + N] of a wider seeded buffer whose other columns must come back bit-unchanged."""

    def __init__(self, M, N, C0, win, g, kind):
        body = C0 if C0 is not None else torch.full((M, N), NAN)
        if win:
            self.wide0 = draw((M, N + 7), kind, g)
            self.wide0[:, 3:3 + N] = body
            self.wide = dev(self.wide0)
            self.C = self.wide[:, 3:3 + N]
        else:
            self.wide0, self.C = None, dev(body)
        self.N = N

    def verify(self, ref, kind, what):
        compare(self.C, ref, kind, what)
        if self.wide0 is not None:
            w = self.wide.cpu()
            assert torch.equal(w[:, :3], self.wide0[:, :3]) and torch.equal(w[:, 3 + self.N:], self.wide0[:, 3 + self.N:]), \
                f"{what}: columns outside the window changed"


def lib_gemm(c, A, A2, B, C, bias, tile):
    """dv3_gemm_f32 through ctypes, arguments as ops.gemm passes them -> the return code."""
    from dv3hip import _lib

    ta, tb = ORIENT[c["o"]]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    ld = lambda t: 0 if t is None else (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))
    rc = _lib.load().dv3_gemm_f32(ta, tb, c["M"], c["N"], c["K1"] + c["K2"], ptr(A), ld(A), ptr(A2), ld(A2), c["K1"],
                                  ptr(B), ld(B), ptr(C), ld(C), ptr(bias), {False: 0, True: 1, "atomic": 2}[c["acc"]], tile,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def run_case(ops, c, kind, via="ops"):
    """One row: the launch(es), the result against the float64 reference (twice: C0 + g, then C0 + 2 g), the window's
    surroundings, and -- where the row names them -- the profile keys of the call."""
    ta, tb = ORIENT[c["o"]]
    A, A2, B, bias, C0 = operands(c, kind)
    g = gen(seed_of(c, kind) + 1)
    out = Out(c["M"], c["N"], C0, c["win"], g, kind)
    Ad, A2d, Bd = place(A, c["lay"]), place(A2, c["lay"]), place(B, c["lay"])
    bd = None if bias is None else dev(bias)
    what = f"{case_id(c)} {kind}"
    keys = c["claims"].get("keys") if via == "ops" else None
    for k in range(1, 3 if c["twice"] else 2):
        if via == "lib":
            assert lib_gemm(c, Ad, A2d, Bd, out.C, bd, c["tile"]) == 0, what
        else:
            if keys is not None:
                ops.PROFILE.start()
                ops.PROFILE.by_shape = False
            ops.gemm(Ad, Bd, out.C, transA=bool(ta), transB=bool(tb), A2=A2d, bias=bd, accumulate=c["acc"], tile=c["tile"])
            if keys is not None:
                got = [(key, rec["launches"]) for key, rec in ops.PROFILE.stop().items()]
                assert got == [kk if isinstance(kk, tuple) else (kk, 1) for kk in keys], (what, got)
        ref = reference(A, A2, B, bias, C0, ta, tb, times=k)
        out.verify(ref, kind, what + (f" call {k}" if c["twice"] else ""))


# ============================================================================================== A: the k-major engine
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("o", list(ORIENT))
@pytest.mark.parametrize("tile", ENGINE_TILES)
def test_kmajor_engine(ops, tile, o, kind):
    for c in ENGINE[(tile, o)]:
        run_case(ops, c, kind)


# ============================================================================================ B: the few-row kernels
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", SKINNY_ROWS, ids=case_id)
def test_few_row_kernel(ops, c, kind):
    run_case(ops, c, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", NARROW_ROWS, ids=case_id)
def test_narrow_output_kernel(ops, c, kind):
    run_case(ops, c, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", NN64_ROWS, ids=case_id)
def test_few_row_nn64_kernel(ops, c, kind):
    run_case(ops, c, kind)


# ======================================================================================= C, D: register-direct kernels
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", DIRECT_ROWS, ids=case_id)
def test_register_direct_kernel(ops, c, kind):
    run_case(ops, c, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", TN_ROWS, ids=case_id)
def test_register_direct_weight_gradient(ops, c, kind):
    run_case(ops, c, kind)


# ========================================================================================== E: k-contiguous LDS tiles
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tile", list(L16))
def test_kcontiguous_lds_tiles(ops, tile, kind):
    for c in L16_CASES[tile]:
        run_case(ops, c, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", AUTO_ROWS, ids=case_id)
def test_kcontiguous_lds_tile_by_size(ops, c, kind):
    run_case(ops, c, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nsplit", SPLIT_NS)
def test_gemm_split(ops, nsplit, kind):
    """ops.gemm_split: columns [0, nsplit) to C, the rest to a strided C2, all four (accumulate, accumulate2)."""
    M, n2, K = SPLIT_SHAPE
    g, A, W = split_operands(nsplit, kind)
    ref = A.double() @ W.double().t()
    Ad, Wd = dev(A), dev(W)
    assert ops.gemm_split_ok(Ad, Wd)
    for acc in (False, True):
        for acc2 in (False, True):
            C10 = draw((M, nsplit), kind, g) if acc else None
            C20 = draw((M, n2), kind, g) if acc2 else None
            o1, o2 = Out(M, nsplit, C10, False, g, kind), Out(M, n2, C20, True, g, kind)
            ops.gemm_split(Ad, Wd, o1.C, o2.C, accumulate=acc, accumulate2=acc2)
            what = f"gemm_split nsplit {nsplit} acc {acc} acc2 {acc2} {kind}"
            o1.verify(ref[:, :nsplit] + (C10.double() if acc else 0), kind, what + " C")
            o2.verify(ref[:, nsplit:] + (C20.double() if acc2 else 0), kind, what + " C2")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_weight_gradients(ops, kind):
    """The grouped grid on GROUP_ROWS: the products gemm_group.takes() run as ONE launch, the others as launches of their
    own (profile keys), every C against C0 + A^T B; row strides wider than the matrices."""
    trip = [(a, b, c0, place(a, "odd"), place(b, "wide4"), place(c0, "odd")) for a, b, c0 in group_operands(kind)]
    ops.PROFILE.start()
    ops.PROFILE.by_shape = False
    with ops.gemm_group():
        for a, b, c0, ad, bd, cd in trip:
            ops.gemm(ad, bd, cd, transA=True, transB=False, accumulate=True)
    keys = {k: v["launches"] for k, v in ops.PROFILE.stop().items()}
    single = [r for r in GROUP_ROWS if not r[3]]
    want = {"gemm_tn_grouped_kernel<64x64x32>": 1}
    for M, N, K, _ in single:
        key = py_route(G(-1, "TN", M, N, K, acc=True))[0][0]
        want[key] = want.get(key, 0) + 1
    assert keys == want, (keys, want)
    for (M, N, K, grouped), (a, b, c0, ad, bd, cd) in zip(GROUP_ROWS, trip):
        compare(cd, c0.double() + a.double().t() @ b.double(), kind, f"grouped {M}x{N}x{K} {kind} (grouped: {grouped})")
        assert bool((cd._base[:, N:] == PAD).all()), "padding of C changed"


# ============================================================================================ F: ops.gemm's own routing
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", ROUTE_ROWS, ids=case_id)
def test_ops_gemm_routing(ops, c, kind):
    run_case(ops, c, kind)


# ========================================================================================= G: the library's own chooser
@pytest.mark.gpu
@pytest.mark.parametrize("c", LIB_ROWS, ids=case_id)
def test_library_chooser(ops, c):
    run_case(ops, c, "int", via="lib")


@pytest.mark.gpu
def test_library_rejections(ops):
    """Calls that return DV3_ERR_ARG before any launch: C stays NaN."""
    from dv3hip import _lib

    for what, tile, o, M, N, K1, K2, bias in REJECT_ROWS:
        c = G(tile, o, M, N, K1, K2, bias=bias)
        A, A2, B, b, _ = operands(c, "int")
        C = torch.full((M, N), NAN, device="cuda")
        assert lib_gemm(c, dev(A), None if A2 is None else dev(A2), dev(B), C, None if b is None else dev(b), tile) == ERR_ARG, what
        assert bool(torch.isnan(C).all()), what
    M, N, K = 40, 72, 32
    A, W = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda")
    C, C2 = torch.full((M, 24), NAN, device="cuda"), torch.full((M, 48), NAN, device="cuda")
    rc = _lib.load().dv3_gemm_split_f32(M, N, K, A.data_ptr(), K, W.data_ptr(), K, C.data_ptr(), 24, 0, C2.data_ptr(), 48, 24,
                                        0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == ERR_ARG and bool(torch.isnan(C).all()) and bool(torch.isnan(C2).all()), "gemm_split with nsplit % 16 != 0"
