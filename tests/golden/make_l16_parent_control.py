#!/usr/bin/env python3
"""Recording of the k-contiguous LDS tile kernels (gemm_l16_kernel, conv_s2_l16_kernel) as they were BEFORE their K loop
moved into csrc/l16_tile.h (commit 37db22f, "Pipeline the k-contiguous LDS tile loop and trim its epilogues"), for the
control test tests/test_l16_loop_gpu.py::test_l16_matches_parent_recording.  Since that move the serial and the
pipelined loop are one piece of shared code: the development library's serial loop can no longer show an error both
have, and the exact-arithmetic tests cannot see a changed order of summation.  Needs an MI355X and a built checkout
of that commit:

    git worktree add <dir> 37db22f && (cd <dir> && python __graft_entry__.py)
    python <this file> <dir> <repository>/tests/golden/l16_parent.npz

Inputs are randn of a seeded CPU generator (weights scaled by 1 / sqrt(K)) and are stored beside the outputs.  Two
files, each below the 1 MiB a committed file may have: <out> holds the GEMM cases, <out stem>_conv.npz the
convolutions.  Data only.  The test imports the case functions below, so both sides run the same calls."""
import math
import os
import sys

import numpy as np
import torch

L16_TILES = (12, 13, 14, 15, 16, 17)  # 64x96, 64x64, 32x64, 128x128, 128x64, 64x128
# A [130, 96], W [136, 96]: an edge tile in both directions on every tile shape.  (K1, K2) as leading-column slices:
# nk = 1 (the drain alone), 2, 3, and the [A | A2] seam
GEMM_K = ((32, 0), (64, 0), (96, 0), (32, 64))
# (transposed, Nimg, H, W, Co), Ci = 32; the last convT: a spatial size that is no power of two (general row decode)
CONV = ((False, 3, 8, 8, 64), (False, 3, 8, 8, 96), (False, 2, 12, 20, 128),
        (True, 3, 4, 4, 128), (True, 3, 4, 4, 96), (True, 2, 3, 5, 128))
CI = 32


def make_inputs():
    g = torch.Generator().manual_seed(3706)
    randn = lambda *s: torch.randn(*s, generator=g)
    gemm = {"A": randn(130, 96), "W": randn(136, 96) / math.sqrt(96), "b": randn(136), "C0": randn(130, 136)}
    # w: every conv weight is a slice of it (conv K = 16 Ci = 512; convT K = 4 Ci: used doubled); x, y0: every input /
    # accumulate base is a leading slice, reshaped
    conv = {"w": randn(128, CI, 4, 4) / math.sqrt(16 * CI), "x": randn(2 * 12 * 20 * CI), "y0": randn(3 * 8 * 8 * 128),
            "cb": randn(128)}
    return gemm, conv


def gemm_cases(ops, d, tile):
    """name -> output of every GEMM case on one tile: all with bias and accumulate, (96, 0) also with neither."""
    A, W, b, C0 = (d[k].cuda() for k in ("A", "W", "b", "C0"))
    out = {}
    for K1, K2 in GEMM_K:
        for plain in ((False, True) if (K1, K2) == (96, 0) else (False,)):
            C = C0.clone()
            ops.gemm(A[:, :K1], W[:, :K1 + K2], C, A2=A[:, K1:K1 + K2] if K2 else None, bias=None if plain else b,
                     accumulate=not plain, tile=tile)
            out[f"gemm {K1}+{K2}" + (" plain" if plain else "")] = C
    return out


def split_case(ops, d):
    """[C | C2] with n1 = 64, K = 96, accumulate (True, False); the tile is the launcher's own choice."""
    C0 = d["C0"].cuda()
    C, C2 = C0[:, :64].contiguous(), C0[:, 64:].contiguous()
    ops.gemm_split(d["A"].cuda(), d["W"].cuda(), C, C2, accumulate=True, accumulate2=False)
    return {"split C": C, "split C2": C2}


def conv_cases(ops, d):
    """name -> output; every case accumulates, convT with bias and out_add = 0.5."""
    out = {}
    for tr, n, h, w, co in CONV:
        oh, ow = (2 * h, 2 * w) if tr else (h // 2, w // 2)
        x = d["x"][:n * h * w * CI].view(n, h, w, CI).cuda()
        y = d["y0"][:n * oh * ow * co].view(n, oh, ow, co).cuda()
        if tr:
            wt = (2.0 * d["w"][:co]).transpose(0, 1).contiguous().cuda()  # [Ci, Co, 4, 4]
            wp = ops.pack_conv_weight(wt, torch.empty(4, co, 4 * CI, device="cuda"), transposed=True)
            ops.convT_s2_fwd(x, wp, y, Ci=CI, Co=co, bias=d["cb"][:co].cuda(), out_add=0.5, accumulate=True)
        else:
            wp = ops.pack_conv_weight(d["w"][:co].cuda(), torch.empty(co, 16 * CI, device="cuda"), transposed=False)
            ops.conv_s2_fwd(x, wp, y, Ci=CI, Co=co, accumulate=True)
        out[f"{'convT' if tr else 'conv'} {n}x{h}x{w} {CI}->{co}"] = y
    return out


def conv_path(gemm_path):
    return gemm_path[:-len(".npz")] + "_conv.npz"


def load(path):
    with np.load(path) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def main():
    root, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    sys.path[:0] = [root, os.path.join(root, "dreamerv3-torch_amd")]
    import dv3hip
    from dv3hip import ops

    assert os.path.abspath(dv3hip.__file__).startswith(root), dv3hip.__file__
    assert out.endswith(".npz")
    gemm_in, conv_in = make_inputs()
    per_tile = [gemm_cases(ops, gemm_in, tile) for tile in L16_TILES]
    for got in per_tile[1:]:
        assert all(torch.equal(got[k], per_tile[0][k]) for k in per_tile[0]), "the parent's six tiles do not agree"
    gemm_out = dict(per_tile[0], **split_case(ops, gemm_in))
    conv_out = conv_cases(ops, conv_in)
    assert not set(gemm_in) & set(gemm_out) and not set(conv_in) & set(conv_out)
    for path, arrays in ((out, dict(gemm_in, **gemm_out)), (conv_path(out), dict(conv_in, **conv_out))):
        np.savez_compressed(path, **{k: v.cpu().numpy() for k, v in arrays.items()})
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
