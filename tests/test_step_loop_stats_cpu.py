"""scripts/step_loop_stats.py on a short hand-written listing: the step loop is the largest
span closed by a backward branch, its segments end at the barriers, and instructions are
classified by mnemonic prefix.  No kernel is compiled."""
import importlib.util
import tempfile
from pathlib import Path

SCRIPT = Path(__file__).resolve().parents[1] / "scripts" / "step_loop_stats.py"

LISTING = """\
	.text
_Z9other_fnv:                           ; @_Z9other_fnv
	s_endpgm
.Lfunc_end0:
_Z4toy_stepPf:                          ; @_Z4toy_stepPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
.LBB1_1:                                ; =>This Loop Header
	v_fma_f32 v1, v2, v3, v1
	v_mfma_f32_16x16x4_f32 a[0:3], v4, v5, a[0:3]
	s_nop 5
	v_accvgpr_read_b32 v6, a0
	ds_write_b32 v7, v6
	s_waitcnt lgkmcnt(0)
	s_barrier
	v_readfirstlane_b32 s2, v6
	s_cmp_lg_u32 s2, 0
	s_cbranch_scc1 .LBB1_3
; %bb.2:
	buffer_store_dwordx4 v[8:11], v12, s[8:11], 0 offen
.LBB1_3:
	ds_read_b64 v[14:15], v7
	s_barrier
	s_add_i32 s3, s3, 1
	s_cmp_lt_i32 s3, s6
	s_cbranch_scc1 .LBB1_1
; %bb.4:
	global_store_dword v0, v1, s[0:1]
	s_endpgm
.Lfunc_end1:
"""


def _mod():
    spec = importlib.util.spec_from_file_location("step_loop_stats", SCRIPT)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_segments_and_classes():
    st = _mod().stats(LISTING, "toy_step")
    assert st["kernel"] == "_Z4toy_stepPf"
    assert st["kernel_instructions"] == 20
    assert st["loop_instructions"] == 16  # .LBB1_1 .. the branch back to it; the prologue and epilogue are outside
    segs = st["segments"]
    assert [s["instructions"] for s in segs] == [7, 6, 3]
    assert segs[0] == {"instructions": 7, "VALU": 1, "MFMA": 1, "nop": 1, "AGPR": 1, "LDS": 1, "wait": 1, "barrier": 1}
    assert segs[1] == {"instructions": 6, "lane": 1, "SALU": 1, "branch": 1, "VMEM": 1, "LDS": 1, "barrier": 1}
    assert segs[2] == {"instructions": 3, "SALU": 2, "branch": 1}
    assert st["classes"] == {"VALU": 1, "MFMA": 1, "lane": 1, "AGPR": 1, "LDS": 2, "VMEM": 1, "wait": 1, "nop": 1,
                             "barrier": 2, "branch": 2, "SALU": 3}
    assert st["branches_seg2_4"] == 2


def test_forward_branch_closes_no_loop():
    m = _mod()
    ins, labels = m.parse(LISTING.split("\n"))
    lo, hi = m.step_loop(ins, labels)
    assert ins[lo][0] == "v_fma_f32" and ins[hi] == ("s_cbranch_scc1", ".LBB1_1")


def test_report_prints_a_row_per_segment(capsys):
    with tempfile.NamedTemporaryFile("w", suffix=".s") as f:
        f.write(LISTING)
        f.flush()
        assert _mod().main([f.name, "toy_step"]) == 0
    out = capsys.readouterr().out
    assert "branches in segments 2-4: 2" in out
    assert sum(ln.split()[0] in ("1", "2", "tail") for ln in out.splitlines() if ln.split()) == 3
