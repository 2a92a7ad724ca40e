"""The ledger of float64 / exact kernel comparisons, and the reachability of the fused, ensemble and column-sum kernels.

1. LEDGER maps every entry point declared in include/dv3hip.h to the test file that compares it with a float64 (or
   exact) reference at its dispatch edges, or to the word `plumbing` with a reason.  The test fails when the header gains
   a symbol the table lacks, and when the named file mentions neither the symbol nor its dv3hip.ops wrapper: the next
   kernel cannot arrive without a comparison of its own.
2. A copy of the host dispatch of csrc/fusedops.hip, csrc/ensops.hip and dv3_colsum (csrc/headops.hip): the cases of
   tests/test_fused_f64_gpu.py and tests/test_ens_f64_gpu.py must land on the instantiations they are there for and, together,
   reach every instantiation of the shipped library (the runtime-activation forms counted once per kernel).
   THE COPY MUST BE UPDATED TOGETHER WITH THE THRESHOLDS IN THE .hip FILES.
"""
import os
import re

from dv3hip import _lib
from tests import test_ens_f64_gpu as TE
from tests import test_fused_f64_gpu as TF

TESTS = os.path.dirname(os.path.abspath(__file__))
OPS_PY = os.path.join(os.path.dirname(TESTS), "dreamerv3-torch_amd", "dv3hip", "ops.py")

ROW, LN, CONV, GEMM = "test_row_kernels_f64_gpu.py", "test_ln_gru_f64_gpu.py", "test_conv_f64_gpu.py", "test_gemm_f64_gpu.py"
FUSED, ENS, NONORM, GAUSS = "test_fused_f64_gpu.py", "test_ens_f64_gpu.py", "test_nonorm_kernels_gpu.py", "test_gauss_kernels_gpu.py"
P = lambda why: ("plumbing", why)

LEDGER = {
    "dv3_version": P("ABI version number"),
    "dv3_dev_switches": P("reports whether the library was built with the development switches"),
    "dv3_device_cu_count": P("device query"),
    "dv3_stream_create_cu_masked": P("stream creation (CU mask)"),
    "dv3_stream_destroy": P("stream destruction"),
    "dv3_rng_advance": P("adds a host integer to the Philox offset; no arithmetic to compare"),
    "dv3_fill_normal": P("Philox stream: no value reference (its statistics are tested in tests/test_gauss_kernels_gpu.py)"),
    "dv3_conv_s2_wgrad_tile_scratch": P("host-side size query of dv3_conv_s2_wgrad_tile's scratch"),
    "dv3_gemm_f32": GEMM, "dv3_gemm_split_f32": GEMM, "dv3_gemm_tn_grouped_f32": GEMM, "dv3_gemm_sample_f32": FUSED,
    "dv3_ln_act_fwd": LN, "dv3_ln_act_bwd": LN, "dv3_ln_act_bwd_ws": LN, "dv3_gru_fwd": LN, "dv3_gru_fwd_blend": LN,
    "dv3_gru_bwd": LN, "dv3_act_fwd": NONORM, "dv3_act_bwd": NONORM, "dv3_gru_nonorm_fwd": NONORM,
    "dv3_gru_nonorm_fwd_blend": NONORM, "dv3_gru_nonorm_bwd": NONORM,
    "dv3_onehot_sample_fwd": ROW, "dv3_onehot_sample_fwd_blend": FUSED, "dv3_onehot_sample_fwd_ex": ROW,
    "dv3_onehot_st_bwd": ROW, "dv3_onehot_ent_logp_fwd": ROW, "dv3_onehot_ent_logp_bwd": ROW, "dv3_kl_fwd": ROW,
    "dv3_kl_bwd": ROW, "dv3_gauss_head_fwd": GAUSS, "dv3_gauss_head_bwd": GAUSS, "dv3_gauss_kl_fwd": GAUSS,
    "dv3_gauss_kl_bwd": GAUSS, "dv3_disc_mode_fwd": ROW, "dv3_disc_mode_bwd": ROW, "dv3_disc_logprob_fwd": ROW,
    "dv3_disc_logprob_bwd": ROW, "dv3_bernoulli_logprob_fwd": ROW, "dv3_bernoulli_logprob_bwd": ROW,
    "dv3_image_to_f32": "test_kernels_gpu.py",  # (exact: u8 / 255 - 0.5 is one rounding)
    "dv3_mse_image": ROW, "dv3_transpose01": ROW, "dv3_concat6": ROW, "dv3_colsum": FUSED, "dv3_colsum_grouped": FUSED,
    "dv3_tanh_fwd": ROW, "dv3_tanh_bwd": ROW, "dv3_pack_conv_weight": CONV, "dv3_im2col_s2": CONV, "dv3_conv_s2_fwd": CONV,
    "dv3_convT_s2_fwd": CONV, "dv3_conv_s2_wgrad_tile": CONV, "dv3_conv_s2_wgrad": CONV, "dv3_conv_s2_c3_fwd": CONV,
    "dv3_convT_s2_c3_fwd": CONV, "dv3_symlog": ROW, "dv3_symlog_mse": ROW, "dv3_actor_normal_fwd": ROW,
    "dv3_actor_normal_logp": ROW, "dv3_actor_normal_bwd": ROW, "dv3_lambda_return_fwd": ROW, "dv3_lambda_return_bwd": ROW,
    "dv3_dot_accumulate": ROW, "dv3_actor_loss": ROW, "dv3_scale_neg": ROW, "dv3_reset_blend": ROW,
    "dv3_reset_blend_bwd": ROW, "dv3_obs_blend": ROW, "dv3_obs_blend_bwd": ROW, "dv3_obs_carry_st_bwd": ROW,
    "dv3_sumsq_accumulate": ROW, "dv3_sumsq_ordered": ROW, "dv3_adam_step": ROW, "dv3_axpby": ROW,
    "dv3_quantile2_ema": FUSED, "dv3_tensorstats": FUSED, "dv3_tensorstats_multi": FUSED,
    "dv3_onehot_sample_linear_ln_fwd": FUSED, "dv3_scan_ln_gemm_fwd": LN, "dv3_scan_ln_gemm_fwd_ex": LN,
    "dv3_scan_gru_factors": LN, "dv3_scan_grubwd_gemm": LN, "dv3_scan_ln_factors": LN, "dv3_scan_ln_factors_ex": LN,
    "dv3_scan_lnbwd_gemm": LN, "dv3_scan_carry_st_gemm": LN, "dv3_onehot_linear_ln_fwd": FUSED, "dv3_actor_head_fwd": FUSED,
    "dv3_actor_head_fwd_ex": FUSED, "dv3_transpose2d": FUSED, "dv3_transpose2d_many": FUSED, "dv3_onehot_to_idx": FUSED,
    "dv3_onehot_wgrad": "test_onehot_wgrad_gpu.py", "dv3_ens_gemm_f32": ENS, "dv3_ens_ln_act_fwd": ENS,
    "dv3_ens_ln_act_bwd": ENS, "dv3_ens_ln_act_fwd_ex": ENS, "dv3_ens_ln_act_bwd_ex": ENS, "dv3_ens_colsum": ENS,
    "dv3_ens_regress_loss": ENS, "dv3_ens_disag_fwd": ENS, "dv3_ens_disag_bwd": ENS, "dv3_ens_pack_rows": "test_ens_pack_gpu.py",
}


def wrappers_of(sym, ops_text):
    """Names of the dv3hip.ops functions (or classes) whose body names the symbol."""
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"^(?:def|class) (\w+)", ops_text, flags=re.M)]
    out = set()
    for m in re.finditer(r'"%s"' % sym, ops_text):
        before = [n for p, n in heads if p < m.start()]
        if before:
            out.add(before[-1])
    return out


def test_every_entry_point_has_a_float64_comparison_or_a_reason():
    syms = set(_lib.parse_header())
    assert syms - set(LEDGER) == set(), f"entry points without a ledger entry: {sorted(syms - set(LEDGER))}"
    assert set(LEDGER) - syms == set(), f"ledger entries the header no longer declares: {sorted(set(LEDGER) - syms)}"
    ops_text = open(OPS_PY).read()
    for sym, entry in LEDGER.items():
        if isinstance(entry, tuple):
            assert entry[0] == "plumbing" and len(entry[1]) > 10, sym
            continue
        path = os.path.join(TESTS, entry)
        assert os.path.exists(path), (sym, entry)
        text = open(path).read()
        names = [sym] + [f"ops.{w}" for w in wrappers_of(sym, ops_text)]
        assert any(re.search(re.escape(n) + r"\b", text) for n in names), f"{entry} mentions none of {names}"


# ------------------------------------------------------------------------------------------------- the dispatch copy
def act_code(act):
    return {False: 0, True: 1, TF.RT_ACT: 5}[act]


def ol_route(N, ldw, ldpre, ldbase, ldy, act):
    """dv3_onehot_linear_ln_fwd (ldbase / ldy: None when the operand is absent)."""
    rt = int(act_code(act) > 1)
    vec = N % 256 == 0 and N <= 1024 and ldw % 4 == 0 and ldpre % 4 == 0 and (ldbase is None or ldbase % 4 == 0) and \
        (ldy is None or ldy % 4 == 0)
    return f"ol_vec<{N // 256},smp=0,rt={rt}>" if vec else f"ol_generic<rt={rt}>"


def ol_case_route(c):
    M, N = c["M"], c["N"]
    ld = lambda name: N if M == 1 else TF.ol_ld(c, name)  # (one row: the wrapper passes ld = N)
    ldbase = None if not c["base"] else ld("pre" if c["base"] == "alias" else "base")
    return ol_route(N, ld("w") if c["S"] * c["D"] + c["A2"] > 1 else N, ld("pre"), ldbase, ld("y") if c["y"] else None, c["act"])


def sl_route(N):
    return f"ol_vec<{N // 256},smp=1,rt=0>"


def ah_route(U, act):
    nv = 1 if U <= 64 else 4 if U <= 256 else 8 if U <= 512 else 16
    return f"actor_head<{nv},rt={int(act_code(act) != 1)}>"


def ens_nv(N):
    return 1 if N <= 64 else 2 if N <= 128 else 4 if N <= 256 else 8 if N <= 512 else 16 if N <= 1024 else 32


def colsum_route(R, N):
    return "colsum_narrow" if N <= 32 and R >= 4096 else "colsum_slab"


def test_cases_land_on_the_instantiations_they_name():
    route = {TF.ol_id(c): ol_case_route(c) for c in TF.OL_CASES}
    assert [ol_case_route(c) for c in TF.OL_WIDTHS] == [f"ol_vec<{k},smp=0,rt=0>" for k in (1, 2, 3, 4)] + ["ol_generic<rt=0>"] * 5
    assert all(ol_case_route(c) == "ol_generic<rt=0>" for c in TF.OL_FALLBACK), route
    assert {ol_case_route(c) for c in TF.OL_GROUPS + TF.OL_IDX} == {"ol_vec<1,smp=0,rt=0>", "ol_generic<rt=0>"}
    assert [ol_case_route(c) for c in TF.OL_ROWS] == ["ol_vec<1,smp=0,rt=0>", "ol_generic<rt=0>"] * 2
    assert {ol_case_route(c) for c in TF.OL_FORMS if c["act"] == TF.RT_ACT} == {"ol_vec<3,smp=0,rt=1>", "ol_generic<rt=1>"}
    # both grid caps are passed: 32768 workgroups of the vec kernel, 16384 of the generic one
    assert any(c["M"] > 32768 and ol_case_route(c).startswith("ol_vec") for c in TF.OL_CASES)
    assert any(c["M"] > 16384 and ol_case_route(c).startswith("ol_generic") for c in TF.OL_CASES)
    assert any(c["M"] > 32768 for c in TF.SL_CASES) and any(c["M"] > 4 * 4096 for c in TF.AH_CASES)
    assert any(c["S"] > 32 for c in TF.OL_CASES if ol_case_route(c).startswith("ol_vec"))  # the second MAXB batch
    for U, want in zip(TF.AH_U, (1, 1, 1, 4, 4, 8, 8, 16, 16)):
        assert ah_route(U, True) == f"actor_head<{want},rt=0>", U
    assert [TF.o2i_group(D) for D in TF.O2I_D] == [4, 4, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert [ens_nv(N) for N in TE.ELN_N] == [1, 1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert any(c["M"] > 64 * 4 for c in TE.ELN_CASES)  # the backward's row loop takes a second trip
    assert [colsum_route(R, N) for R, N, _ in TF.CS_CASES] == ["colsum_slab"] * 6 + ["colsum_narrow"] * 6
    assert any(R * N > 1024 * 256 * 64 for R, N, _ in TF.CS_CASES)  # past the narrow kernel's 1024 workgroups
    assert any(-(-R // 64) > 64 for R, N, _ in TF.CS_CASES if colsum_route(R, N) == "colsum_slab")  # the 64-slab cap
    # actor head: OB = 12 (NV <= 8) and OB = 6 (NV = 16) each see a full batch, a remainder and a second batch
    for U, ob in ((512, 12), (1024, 6)):
        nouts = {(1 if c["onehot"] else 2) * c["A"] for c in TF.AH_GRID[U]}
        assert any(n == ob for n in nouts) and any(n < ob for n in nouts) and any(n > ob and n % ob for n in nouts), (U, nouts)


def test_cases_reach_every_instantiation_of_the_shipped_library():
    """Every template instantiation the host code of csrc/fusedops.hip and csrc/ensops.hip can launch (and the three
    column-sum kernels) is reached by a case; of the runtime-activation (RT) forms one per kernel is required."""
    reached = {ol_case_route(c) for c in TF.OL_CASES} | {sl_route(c["N"]) for c in TF.SL_CASES}
    reached |= {ah_route(c["U"], c["act"]) for c in TF.AH_CASES}
    reached |= {f"onehot_to_idx<{TF.o2i_group(D)}>" for D in TF.O2I_D}
    reached |= {f"ens_ln<{ens_nv(c['N'])},rt={int(act_code(c['act']) != 1)}>" for c in TE.ELN_CASES}
    reached |= {f"ens_gemm<{c['o']}>" for c in TE.EG_CASES} | {colsum_route(R, N) for R, N, _ in TF.CS_CASES}
    need = ({f"ol_vec<{k},smp={s},rt=0>" for k in (1, 2, 3, 4) for s in (0, 1)} | {"ol_generic<rt=0>"} |
            {f"actor_head<{nv},rt=0>" for nv in (1, 4, 8, 16)} | {f"onehot_to_idx<{g}>" for g in (4, 8, 16, 32, 64)} |
            {f"ens_ln<{nv},rt=0>" for nv in (1, 2, 4, 8, 16, 32)} | {f"ens_gemm<{o}>" for o in ("NT", "NN", "TN")} |
            {"colsum_slab", "colsum_narrow"})
    assert need - reached == set(), sorted(need - reached)
    for kernel in ("ol_vec<", "ol_generic<", "actor_head<", "ens_ln<"):  # one RT form per kernel
        assert any(r.startswith(kernel) and r.endswith("rt=1>") for r in reached), kernel
