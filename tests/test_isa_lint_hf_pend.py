"""tools/check_rr_waits.py on the HF instantiations with the pending-pattern hand-off (lstm_rr_hfp_kernel): the run over the real ISA is
tests/test_isa_lint.py's (the tool's exit status covers the new checks: eight-leaf looks, marks, no flag drain, no scratch); here the check
itself is shown to see what it must see, on synthetic listings."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("check_rr_waits", os.path.join(ROOT, "tools", "check_rr_waits.py"))
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

NAME = "_Z18lstm_rr_hfp_kernelILi8ELi2EEv8RRParams"


def listing(look, extra="", scratch=0, n=32):
    body = "\n".join(look for _ in range(n))
    return ("\n%s:\n%s\n%s\n.Lfunc_end0:\n.amdhsa_kernel %s\n .amdhsa_private_segment_fixed_size %d\n.end_amdhsa_kernel\n"
            % (NAME, body, extra, NAME, scratch))


GOOD = "v_max3_u32 v1, v10, v11, v12\nv_max3_u32 v2, v13, v14, v15\nv_max3_u32 v3, v1, v2, v16\nv_max_u32_e32 v4, v3, v17\nv_cmp_eq_u32_e32 vcc, -1, v4"
SEVEN = "v_max3_u32 v1, v10, v11, v12\nv_max3_u32 v2, v13, v14, v15\nv_max3_u32 v3, v1, v2, v16\nv_cmp_eq_u32_e32 vcc, -1, v3"


def test_a_look_over_eight_words_passes():
    assert tool.check_pending(listing(GOOD), tool.HFP, 8, 32) == (0, 32)


def test_a_look_that_misses_a_word_too_few_looks_a_drain_or_scratch_are_defects(capsys):
    assert tool.check_pending(listing(SEVEN), tool.HFP, 8, 32)[0] == 32
    assert tool.check_pending(listing(GOOD, n=31), tool.HFP, 8, 32)[0] == 1
    assert tool.check_pending(listing(GOOD, extra=";ASMSTART\ns_waitcnt vmcnt(2)\n;ASMEND"), tool.HFP, 8, 32)[0] == 1
    assert tool.check_pending(listing(GOOD, scratch=16), tool.HFP, 8, 32)[0] == 1
    capsys.readouterr()


def test_the_kh4_pattern_does_not_take_the_hf_kernels_for_its_own():
    assert tool.check_pending(listing(GOOD)) == (0, 0)
