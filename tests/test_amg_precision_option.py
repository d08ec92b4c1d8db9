"""NSK_OPT_AMG_PRECISION in the public header, the Python wrapper and the kernel rule of the V-cycle (no GPU)."""
import ctypes as C
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "nsk.h")) as f:
        return f.read()


def test_option_value_matches_the_header_and_is_documented():
    from navier_stokes_solver_amd import solver as S
    h = _header()
    m = re.search(r"NSK_OPT_AMG_PRECISION\s*=\s*(\d+)\s*,?\s*/\*(.*?)\*/", h, re.S)
    assert m, "NSK_OPT_AMG_PRECISION is not declared with a comment in include/nsk.h"
    assert S.OPT_AMG_PRECISION == int(m.group(1)) == 20
    doc = " ".join(m.group(2).split())
    for what in ("64", "32", "V-cycle", "A LABELLED DEVIATION from the reference", "NSK_AMG_PRECISION", "-48", "-61",
                 "What stays double", "set-up", "dense inverse", "Chebyshev", "nsk_amg_value_bytes", "next nsk_setup_preconditioner"):
        assert what.lower() in doc.lower(), what
    # the two older options no longer say the AMG has no switch
    for opt in ("NSK_OPT_FACTOR_PRECISION", "NSK_OPT_INNER_MATRIX_PRECISION"):
        d = re.search(opt + r"\s*=\s*\d+\s*,?\s*/\*(.*?)\*/", h, re.S).group(1)
        assert "NSK_OPT_AMG_PRECISION" in d, opt
    ids = re.findall(r"^\s*NSK_OPT_\w+\s*=\s*(\d+)", h, re.M)
    assert len(ids) == len(set(ids))


def test_export_is_declared_and_listed():
    from navier_stokes_solver_amd import solver as S
    h = _header()
    assert re.search(r"int\s+nsk_amg_value_bytes\s*\(\s*nsk_handle\s+h\s*,\s*int32_t\s*\*\s*bytes\s*\)", h)
    assert "nsk_amg_value_bytes" in S.EXPORTS
    assert callable(S.LinearSolver.amg_value_bytes)
    m = re.search(r"int nsk_time_op\(", h)
    doc = h[h.rfind("/*", 0, m.start()):m.start()]
    assert re.search(r"\b57\b", doc) and "V-cycle" in doc


def test_out_of_range_error_code_is_listed():
    """-48 keeps the line the inner-matrix option's test reads and names the AMG case beside it."""
    h = _header()
    m = re.search(r"^\s*\*\s*-48\b(.*)$", h, re.M)
    assert m and "NSK_OPT_INNER_MATRIX_PRECISION" in m.group(1) and "fp32" in m.group(1)
    tail = h[m.end():m.end() + 300]
    assert "NSK_OPT_AMG_PRECISION" in tail.split("\n *   -5")[0]


def _lib():
    from navier_stokes_solver_amd import solver as S
    L = S.lib()
    L.nsk_debug_amg_spmv_form.argtypes = [C.c_int] * 6
    L.nsk_debug_spmv_form.argtypes = [C.c_int] * 7
    return L


CSRV, STREAM, STREAM_F32, BLK, BLK_F32 = range(5)


def test_the_rule_of_the_v_cycle_over_all_flags():
    L = _lib()
    seen = set()
    for blk_ok, stream_ok, amg32, use_bsr, mode, al in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)):
        f = L.nsk_debug_amg_spmv_form(blk_ok, stream_ok, amg32, use_bsr, mode, al)
        if not amg32:
            # 64: today's choice — Amg::mv asked for spmv_form(true, false, mode) of the operator
            assert f == L.nsk_debug_spmv_form(blk_ok, stream_ok, 0, 1, 0, mode, 0), (blk_ok, stream_ok, use_bsr, mode, al)
            assert f in (CSRV, STREAM)
            continue
        if blk_ok and use_bsr and al and mode in (0, 2):
            want = BLK_F32
        elif stream_ok:
            want = STREAM_F32
        else:
            want = CSRV
        assert f == want, (blk_ok, stream_ok, use_bsr, mode, al, f)
        seen.add(f)
        # no fp64 stream or block form under 32, no block form for x += P x_c, none on vectors off the pair alignment
        assert f not in (STREAM, BLK)
        if mode == 1 or not al:
            assert f != BLK_F32
    assert seen == {CSRV, STREAM_F32, BLK_F32}


def test_driver_lines_and_documents():
    text = "[nsk] NSK_AMG_PRECISION=32: velocity AMG operators stored in fp32 (deviation from the reference)"
    for rel in (("navier_stokes_solver_amd", "csrc", "cli_main.cpp"), ("navier_stokes_solver_amd", "newton.py")):
        with open(os.path.join(ROOT, *rel)) as f:
            assert text in f.read(), rel
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        d = f.read()
    assert re.search(r"^#+ *5t\b", d, re.M) and "NSK_OPT_AMG_PRECISION" in d
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "NSK_AMG_PRECISION" in f.read()
    with open(os.path.join(ROOT, "scripts", "README.md")) as f:
        assert "time_amg_precision.py" in f.read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "time_amg_precision.py"))
