"""The one rule that chooses a block's SpMV kernel (nsk::spmv_form), through nsk_debug_spmv_form: every input
against the five lines of the rule written out here (no GPU, no handle)."""
import itertools

from navier_stokes_solver_amd import solver as S


def rule(blk_ok, stream_ok, inner32, use_stream, use_bsr, mode, inner):
    if inner and mode == 0 and inner32 == 1 and use_stream and use_bsr and blk_ok:
        return "blk_f32"
    if inner and mode == 0 and inner32 == 2 and use_stream and stream_ok and not (blk_ok and use_bsr):
        return "stream_f32"
    if blk_ok and use_stream and use_bsr and mode == 0:
        return "blk"
    if stream_ok and use_stream:
        return "stream"
    return "csr_vector"


def every_input():
    for flags in itertools.product((0, 1), repeat=5):
        blk_ok, stream_ok, use_stream, use_bsr, inner = flags
        for inner32 in (0, 1, 2):
            for mode in (0, 1, 2):
                yield blk_ok, stream_ok, inner32, use_stream, use_bsr, mode, inner


def test_the_export_is_listed_and_the_names_follow_the_enum():
    assert "nsk_debug_spmv_form" in S.EXPORTS
    assert S.SPMV_FORMS == ("csr_vector", "stream", "stream_f32", "blk", "blk_f32")


def test_every_input_gives_the_form_of_the_written_rule():
    seen = set()
    n = 0
    for args in every_input():
        got = S.spmv_form(*args)
        assert got == rule(*args), (args, got)
        seen.add(got)
        n += 1
    assert n == 2 ** 5 * 3 * 3
    assert seen == set(S.SPMV_FORMS)


def test_only_an_inner_product_reads_an_fp32_copy():
    for args in every_input():
        if not args[6]:
            assert not S.spmv_form(*args).endswith("_f32"), args


def test_y_plus_and_z_minus_products_take_neither_a_blocked_nor_an_fp32_form():
    for args in every_input():
        if args[5] != 0:
            assert S.spmv_form(*args) in ("csr_vector", "stream"), args
