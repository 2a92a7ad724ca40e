"""CPU-side checks of the LayerNorm-free entry points (dv3_act_*, dv3_gru_nonorm_*): declared, exported, bound with the
header's argument types, and their argument rejection returns before any launch (safe to call with no GPU)."""
import ctypes

from dv3hip import _lib

NEW = ["dv3_act_fwd", "dv3_act_bwd", "dv3_gru_nonorm_fwd", "dv3_gru_nonorm_fwd_blend", "dv3_gru_nonorm_bwd"]
ERR_ARG = 10001


def test_entry_points_are_declared_and_exported():
    decls = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in decls, f"{name} not declared in include/dv3hip.h"
        assert hasattr(lib, name), f"{name} not exported by libdv3hip"
    # no LayerNorm operands: neither statistics nor affine parameters nor their gradients
    for name in NEW:
        names = {nm for _, nm in decls[name]}
        assert not names & {"gamma", "beta", "mean", "rstd", "dgamma", "dbeta"}, (name, names)


def test_ops_wrappers_exist():
    from dv3hip import ops

    for fn in ("act_fwd", "act_bwd", "gru_nonorm_fwd", "gru_nonorm_bwd"):
        assert callable(getattr(ops, fn))
    assert ops.ACT_GRID_CAP == 2048


def test_argument_rejection_happens_before_any_launch():
    lib = _lib.load()
    one = 16  # a non-NULL, 16-byte aligned address that is never dereferenced: every call below returns before a launch
    # empty problems are not an error
    assert lib.dv3_act_fwd(None, 0, None, 0, 0, 8, 1, 0, None) == 0
    assert lib.dv3_act_bwd(None, 0, None, 0, None, 0, 0, 8, 1, 0, 0, None) == 0
    assert lib.dv3_gru_nonorm_fwd(None, 0, None, 0, None, 0, 0, 16, None) == 0
    assert lib.dv3_gru_nonorm_bwd(None, 0, None, 0, None, 0, None, 0, None, 0, 0, 16, 0, None) == 0
    # NULL operands
    assert lib.dv3_act_fwd(None, 8, None, 8, 4, 8, 1, 0, None) == ERR_ARG
    assert lib.dv3_act_bwd(None, 8, None, 8, None, 8, 4, 8, 1, 0, 0, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_fwd(None, 48, None, 16, None, 16, 4, 16, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_bwd(None, 16, None, 48, None, 16, None, 48, None, 16, 4, 16, 0, None) == ERR_ARG
    # an activation code outside the table, a row stride below the row length, rows that are no whole images
    assert lib.dv3_act_fwd(one, 8, one, 8, 4, 8, 7, 0, None) == ERR_ARG
    assert lib.dv3_act_fwd(one, 8, one, 8, 4, 8, -1, 0, None) == ERR_ARG
    assert lib.dv3_act_fwd(one, 7, one, 8, 4, 8, 1, 0, None) == ERR_ARG
    assert lib.dv3_act_fwd(one, 8, one, 7, 4, 8, 1, 0, None) == ERR_ARG
    assert lib.dv3_act_fwd(one, 8, one, 8, 4, 8, 1, 3, None) == ERR_ARG
    assert lib.dv3_act_bwd(one, 8, one, 8, one, 7, 4, 8, 1, 0, 0, None) == ERR_ARG
    assert lib.dv3_act_bwd(one, 8, one, 8, one, 8, 4, 8, 1, 3, 0, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_fwd(one, 47, one, 16, one, 16, 4, 16, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_fwd(one, 48, one, 16, one, 15, 4, 16, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_bwd(one, 16, one, 48, one, 16, one, 47, one, 16, 4, 16, 0, None) == ERR_ARG
    # the fused reset blend: the widths dv3_gru_fwd_blend takes, all three blend operands, a 16-byte row stride
    assert lib.dv3_gru_nonorm_fwd_blend(one, 48, one, 16, one, 16, 4, 16, one, one, one, 16, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_fwd_blend(one, 768, one, 256, one, 256, 4, 256, None, one, one, 256, None) == ERR_ARG
    assert lib.dv3_gru_nonorm_fwd_blend(one, 768, one, 256, one, 256, 4, 256, one, one, one, 258, None) == ERR_ARG
    # the LayerNorm entry points keep refusing a NULL gamma: norm=False is not an overload of theirs
    assert lib.dv3_ln_act_fwd(one, 8, None, None, one, 8, None, None, 4, 8, 1, 0, None) == ERR_ARG
    assert lib.dv3_gru_fwd(one, 48, None, None, one, 16, one, 16, one, one, 4, 16, None) == ERR_ARG
