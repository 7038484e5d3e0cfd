"""scripts/kernel_digest.py on two short hand-written listings: listings that differ only in
the ``__hip_cuid_`` symbol compare equal; one changed instruction in one kernel makes them
unequal and names that kernel.  No kernel is compiled."""
import importlib.util
from pathlib import Path

SCRIPT = Path(__file__).resolve().parents[1] / "scripts" / "kernel_digest.py"

LISTING = """\
	.text
	.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
_Z6helperf:                             ; @_Z6helperf
	v_add_f32_e32 v0, v0, v0
	s_setpc_b64 s[30:31]
.Lfunc_end0:
_Z5firstPf:                             ; @_Z5firstPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z5firstPf
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr 2
	.end_amdhsa_kernel
	.text
.Lfunc_end1:
_Z6secondPf:                            ; @_Z6secondPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 1.0
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z6secondPf
		.amdhsa_group_segment_fixed_size 64
		.amdhsa_next_free_vgpr 2
	.end_amdhsa_kernel
	.text
.Lfunc_end2:
	.type	__hip_cuid_0123456789abcdef,@object
	.globl	__hip_cuid_0123456789abcdef
__hip_cuid_0123456789abcdef:
	.byte	0
"""


def _mod():
    spec = importlib.util.spec_from_file_location("kernel_digest", SCRIPT)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_one_digest_per_kernel_and_one_for_the_file(tmp_path, capsys):
    m = _mod()
    kernels, whole = m.digests(LISTING)
    assert list(kernels) == ["_Z5firstPf", "_Z6secondPf"]  # the device function is no kernel
    assert kernels["_Z5firstPf"] != kernels["_Z6secondPf"]
    assert m.main([_write(tmp_path, "a.s", LISTING)]) == 0
    rows = [ln.split() for ln in capsys.readouterr().out.splitlines()]
    assert [r[1] for r in rows] == ["_Z5firstPf", "_Z6secondPf", "*"]
    assert rows[0][0] == kernels["_Z5firstPf"] and rows[2][0] == whole
    assert all(len(r[0]) == 64 for r in rows)


def test_the_cuid_symbol_alone_is_no_difference(tmp_path, capsys):
    m = _mod()
    other = LISTING.replace("0123456789abcdef", "fedcba9876543210")
    assert other != LISTING
    assert m.digests(other) == m.digests(LISTING)
    assert m.main(["--diff", _write(tmp_path, "a.s", LISTING), _write(tmp_path, "b.s", other)]) == 0
    assert capsys.readouterr().out.strip() == "identical"


def test_one_instruction_names_its_kernel(tmp_path, capsys):
    m = _mod()
    other = LISTING.replace("v_mov_b32_e32 v1, 1.0", "v_mov_b32_e32 v1, 2.0")
    assert m.diff(LISTING, other) == ["differs    _Z6secondPf"]
    assert m.main(["--diff", _write(tmp_path, "a.s", LISTING), _write(tmp_path, "b.s", other)]) == 1
    assert capsys.readouterr().out.split() == ["differs", "_Z6secondPf"]


def test_descriptor_kernel_set_and_the_rest_of_the_file(tmp_path):
    m = _mod()
    # the kernel descriptor is part of the kernel's digest
    lds = LISTING.replace("fixed_size 64", "fixed_size 80")
    assert m.diff(LISTING, lds) == ["differs    _Z6secondPf"]
    # a kernel in one listing only
    cut = LISTING[:LISTING.index("_Z6secondPf:")] + LISTING[LISTING.index(".Lfunc_end2:"):]
    assert m.diff(LISTING, cut) == ["only in A  _Z6secondPf"]
    assert m.diff(cut, LISTING) == ["only in B  _Z6secondPf"]
    # a difference outside every kernel still fails the comparison
    fn = LISTING.replace("v_add_f32_e32 v0, v0, v0", "v_mul_f32_e32 v0, v0, v0")
    assert m.diff(LISTING, fn) == ["differs    * (outside the kernels)"]
    assert m.main(["--diff", _write(tmp_path, "a.s", LISTING), _write(tmp_path, "b.s", fn)]) == 1


# the two kernels with a loop each: basic-block labels .LBB<function ordinal>_<block>
# and the comments that name them
LOOPS = LISTING.replace("\tv_mov_b32_e32 v1, 0\n", ".LBB1_1:\n\tv_mov_b32_e32 v1, 0\n\ts_cbranch_scc1 .LBB1_1\n") \
               .replace("\tv_mov_b32_e32 v1, 1.0\n",
                        ".LBB2_1:                                ;   in Loop: Header=BB2_1 Depth=1\n"
                        "\tv_mov_b32_e32 v1, 1.0\n\ts_cbranch_scc1 .LBB2_1\n")


def test_the_function_ordinal_alone_is_no_difference_under_the_mask(tmp_path, capsys):
    m = _mod()
    assert LOOPS.count(".LBB1_1") == 2 and LOOPS.count(".LBB2_1") == 2 and LOOPS.count("=BB2_1") == 1
    other = LOOPS.replace("BB1_", "BB7_").replace(".LBB2_1:        ", ".LBB12_1:       ").replace("BB2_", "BB12_")
    assert m.digests(other, True)[0] == m.digests(LOOPS, True)[0]
    assert m.diff_kernels([LOOPS], [other]) == []
    a, b = _write(tmp_path, "a.s", LOOPS), _write(tmp_path, "b.s", other)
    assert m.main(["--mask-ordinals", "--diff", a, "--", b]) == 0
    assert capsys.readouterr().out.strip() == "identical"
    # the default mode stays byte-exact
    assert m.diff(LOOPS, other) == ["differs    _Z5firstPf", "differs    _Z6secondPf"]
    assert m.main(["--diff", a, b]) == 1
    # the listing form: the kernels' lines agree under the mask only
    rows = []
    for argv in (["--mask-ordinals", a], ["--mask-ordinals", b], [a], [b]):
        capsys.readouterr()
        assert m.main(argv) == 0
        rows.append(capsys.readouterr().out.splitlines()[:2])
    assert rows[0] == rows[1] and rows[2] != rows[3]


def test_a_block_number_or_an_instruction_still_differs_under_the_mask():
    m = _mod()
    block = LOOPS.replace(".LBB2_1", ".LBB2_2")
    assert m.diff_kernels([LOOPS], [LOOPS.replace("=BB2_1", "=BB2_2")]) == ["differs    _Z6secondPf"]
    assert m.diff_kernels([LOOPS], [block]) == ["differs    _Z6secondPf"]
    insn = LOOPS.replace("v_mov_b32_e32 v1, 1.0", "v_mov_b32_e32 v1, 2.0")
    assert m.diff_kernels([LOOPS], [insn]) == ["differs    _Z6secondPf"]


def test_a_kernel_moved_to_a_second_listing_compares_equal(tmp_path, capsys):
    m = _mod()
    i, j = LOOPS.index("_Z6secondPf:"), LOOPS.index(".Lfunc_end2:")
    b1 = LOOPS[:i] + LOOPS[j:]
    b2 = "\t.text\n" + LOOPS[i:j].replace("BB2_", "BB0_")  # the first function of its own listing
    assert list(m.digests(b2)[0]) == ["_Z6secondPf"]
    assert m.diff_kernels([LOOPS], [b1, b2]) == []
    assert m.diff_kernels([LOOPS], [b1]) == ["only in A  _Z6secondPf"]
    files = [_write(tmp_path, n, t) for n, t in (("a1.s", LOOPS), ("b1.s", b1), ("b2.s", b2))]
    assert m.main(["--mask-ordinals", "--diff", files[0], "--", files[1], files[2]]) == 0
    assert capsys.readouterr().out.strip() == "identical"
