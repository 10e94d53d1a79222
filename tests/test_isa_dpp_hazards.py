"""The build-time assembly check's DPP rule (lfsd_amd/isa_check.py: find_dpp_hazards): a DPP instruction needs 2 wait states behind a
vector instruction that wrote its src0 and 5 behind one that wrote EXEC.  The compiler keeps them for its own DPP instructions, not
for the v_fmac_f32_dpp that cpdp_common.h's fmac2_row_bcast writes in an asm statement, so every build is scanned.  Text only: no GPU."""
import pytest

from lfsd_amd import isa_check

FMAC = "\tv_fmac_f32_dpp v71, v48, v4 row_newbcast:10 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
MOV = "\tv_mov_b32_dpp v9, v48 quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
OTHER = "\tv_add_f32_e32 v5, v150, v5\n"


def _fn(body):
    return "\t.text\n_Z6kernelv:\n; %bb.0:\n" + body + "\ts_endpgm\n.Lfunc_end0:\n"


def _kinds(body):
    return [h["kind"] for h in isa_check.find_dpp_hazards(_fn(body))]


@pytest.mark.parametrize("dpp", [FMAC, MOV])
@pytest.mark.parametrize("writer", ["\tv_accvgpr_read_b32 v48, a12\n", "\tv_fma_f32 v48, v1, v2, v3\n", "\tv_mov_b32_e32 v[48:49], v[2:3]\n",
                                    "\tv_swap_b32 v7, v48\n", "\tv_permlane32_swap_b32_e32 v7, v48\n"])
def test_a_writer_of_src0_needs_two_wait_states(dpp, writer):
    assert _kinds(writer + dpp) == ["dpp-src0"]
    assert _kinds(writer + OTHER + dpp) == ["dpp-src0"]
    assert _kinds(writer + OTHER + OTHER + dpp) == []
    assert _kinds(writer + "\ts_nop 0\n" + dpp) == ["dpp-src0"]
    assert _kinds(writer + "\ts_nop 1\n" + dpp) == []
    assert _kinds(writer + ";;#ASMSTART\n\ts_nop 4\n;;#ASMEND\n;;#ASMSTART\n" + dpp + ";;#ASMEND\n") == []


def test_only_src0_and_only_vector_writers_count():
    # src1 and the accumulator are ordinary operands; a load that writes src0 is waited for by s_waitcnt, not by distance
    assert _kinds("\tv_add_f32_e32 v4, v150, v5\n" + FMAC) == []
    assert _kinds("\tv_add_f32_e32 v71, v150, v5\n" + FMAC) == []
    assert _kinds("\tds_read_b32 v48, v3\n\ts_waitcnt lgkmcnt(0)\n" + FMAC) == []
    assert _kinds("\tv_cmp_lt_f32_e32 vcc, v48, v4\n" + FMAC) == []
    # the second instruction of a statement reads what a DPP instruction in front of it wrote as src0: also a vector writer
    assert _kinds("\tv_fmac_f32_dpp v48, v1, v2 row_newbcast:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n" + FMAC) == ["dpp-src0"]
    h = isa_check.find_dpp_hazards(_fn("\tv_accvgpr_read_b32 v48, a12\n" + FMAC))[0]
    assert h["function"] == "_Z6kernelv" and h["writer"] == "v_accvgpr_read_b32 v48, a12" and h["line"] == h["writer_line"] + 1
    assert h["instr"].startswith("v_fmac_f32_dpp v71, v48, v4")


def test_a_vector_write_of_exec_needs_five_wait_states():
    w = "\tv_cmpx_lt_f32_e32 v1, v2\n"
    for n in range(5):
        assert _kinds(w + OTHER * n + FMAC) == ["dpp-exec"], n
    assert _kinds(w + OTHER * 5 + FMAC) == []
    assert _kinds(w + "\ts_nop 3\n" + FMAC) == ["dpp-exec"]
    assert _kinds(w + "\ts_nop 4\n" + FMAC) == []
    assert _kinds("\tv_readfirstlane_b32 exec_lo, v3\n" + OTHER + FMAC) == ["dpp-exec"]
    # a scalar write of EXEC is not this hazard (the join blocks of every divergent region have one)
    assert _kinds("\ts_or_b64 exec, exec, s[0:1]\n" + FMAC) == []


def test_matrix_and_transcendental_results():
    assert _kinds("\tv_rcp_f32_e32 v4, v9\n" + FMAC) == ["dpp-trans"]
    assert _kinds("\tv_rcp_f32_e32 v4, v9\n" + OTHER + FMAC) == []
    m4 = "\tv_mfma_f32_4x4x1_16b_f32 v[68:71], v1, v2, v[68:71]\n"
    m32 = "\tv_mfma_f32_32x32x2_f32 v[0:15], v100, v101, v[0:15]\n"
    assert _kinds(m4 + OTHER * 4 + FMAC) == ["dpp-mfma"] and _kinds(m4 + OTHER * 5 + FMAC) == []
    assert _kinds(m32 + OTHER * 18 + FMAC) == ["dpp-mfma"] and _kinds(m32 + OTHER * 19 + FMAC) == []
    assert _kinds("\tv_mfma_f32_32x32x2_f32 a[0:15], v100, v101, a[0:15]\n" + FMAC) == []       # (accumulation registers are not VGPRs)


def test_every_path_to_the_instruction_counts():
    # the writer sits at the end of a block that BRANCHES to the DPP instruction's block; the fall-through path is clean
    body = ("\tv_accvgpr_read_b32 v48, a12\n\ts_cbranch_vccnz .LBB0_2\n"
            "; %bb.1:\n" + OTHER * 3 +
            ".LBB0_2:\n" + FMAC)
    assert _kinds(body) == ["dpp-src0"]
    assert _kinds(body.replace(".LBB0_2:\n", ".LBB0_2:\n" + OTHER)) == []
    # behind an unconditional branch nothing falls through: the writer in front of the label is on no path
    body = ("\ts_branch .LBB0_3\n.LBB0_9:\n\tv_accvgpr_read_b32 v48, a12\n\ts_branch .LBB0_4\n"
            ".LBB0_3:\n" + FMAC + ".LBB0_4:\n")
    assert _kinds(body) == []
    # a loop: the back edge brings the writer at the bottom in front of the DPP instruction at the top
    loop = ".LBB0_1:\n" + FMAC + OTHER * 3 + "\tv_mov_b32_e32 v48, v5\n\ts_cbranch_scc1 .LBB0_1\n"
    assert _kinds(loop) == ["dpp-src0"]
    assert _kinds(loop.replace("\ts_cbranch_scc1", OTHER + "\ts_cbranch_scc1")) == []
    # the first instruction of a function has no predecessor in the function in front of it
    two = _fn("\tv_mov_b32_e32 v48, v5\n").replace("\ts_endpgm\n", "") + "_Z7kernel2v:\n" + FMAC + "\ts_endpgm\n"
    assert isa_check.find_dpp_hazards(two) == []


def test_find_hazards_reports_both_kinds_and_the_count():
    text = _fn("\tv_accvgpr_read_b32 v48, a12\n" + FMAC + MOV)
    assert [h["kind"] for h in isa_check.find_hazards(text)] == ["dpp-src0", "dpp-src0"]      # (the move reads v48 one instruction later)
    assert isa_check.dpp_count(text) == 2
    assert isa_check.find_hazards(_fn(OTHER)) == [] and isa_check.dpp_count(_fn(OTHER)) == 0
