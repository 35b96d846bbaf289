"""tools/asm_operand_overlap.py: the scan of the emitted gfx950 ISA for inline-assembly inputs that share a register with an
operand the same statement has already written (no GPU: hipcc cross-compiles)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_operand_overlap as scan  # noqa: E402

# msm_digits_kernel as it was compiled before the read-write operands became early-clobber: Fr::from_mont multiplies by
# (1, 0, .., 0), and v33 holds both the literal zero b.v[1] and the statement's carry word
EXCERPT = """\
_ZN3uzk17msm_digits_kernelEPKNS_2FpEPjm: ; @_ZN3uzk17msm_digits_kernelEPKNS_2FpEPjm
\tv_mov_b32_e32 v33, 0
\t;;#ASMSTART
\tv_mad_u64_u32 v[30:31], vcc, v0, v33, v[30:31]
\tv_addc_co_u32_e32 v33, vcc, 0, v33, vcc
\tv_mad_u64_u32 v[30:31], vcc, v1, v33, v[30:31]
\tv_addc_co_u32_e32 v33, vcc, 0, v33, vcc
\t;;#ASMEND
\ts_endpgm
"""


def test_the_overlapped_read_of_the_excerpt_is_reported_and_only_that():
    found, symbols, blocks = scan.scan_text(EXCERPT)
    assert (symbols, blocks) == (1, 1)
    assert [(f.kernel, f.line_no, f.text, f.registers) for f in found] == [
        ("_ZN3uzk17msm_digits_kernelEPKNS_2FpEPjm", 6, "v_mad_u64_u32 v[30:31], vcc, v1, v33, v[30:31]", (33,))]
    # the same block with the literal in a register of its own: nothing to report
    renamed = EXCERPT.replace("vcc, v0, v33,", "vcc, v0, v34,").replace("vcc, v1, v33,", "vcc, v1, v34,")
    assert renamed != EXCERPT and scan.scan_text(renamed)[0] == []


def test_a_carry_chain_reading_a_word_it_has_written_is_reported():
    chain = "k: ; @k\n;;#ASMSTART\nv_add_co_u32_e32 v0, vcc, v0, v8\nv_addc_co_u32_e32 v1, vcc, v1, v0, vcc\n;;#ASMEND\n"
    found = scan.scan_text(chain)[0]
    assert [(f.line_no, f.registers) for f in found] == [(4, (0,))]
    assert scan.scan_text(chain.replace("v1, v0, vcc", "v1, v9, vcc"))[0] == []
    # writes outside an asm block, and other opcodes inside one, are not read
    assert scan.scan_text("k: ; @k\nv_add_co_u32_e32 v0, vcc, v0, v8\nv_addc_co_u32_e32 v1, vcc, v1, v0, vcc\n")[0] == []


@pytest.mark.parametrize("unit", ["srscheck.hip", "synth.hip"])
def test_the_smallest_translation_units_compile_without_overlap(unit):
    (found, symbols, blocks), = scan.scan_units(units=[unit], jobs=1).values()
    assert symbols > 0 and blocks > 0, "no kernel or no inline assembly seen: the scan read nothing"
    assert found == []
