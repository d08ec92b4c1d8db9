"""NSK_OPT_INNER_MATRIX_PRECISION in the public header and in the Python wrapper (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "nsk.h")) as f:
        return f.read()


def test_option_value_matches_the_header_and_is_documented():
    from navier_stokes_solver_amd import solver as S
    h = _header()
    m = re.search(r"NSK_OPT_INNER_MATRIX_PRECISION\s*=\s*(\d+)\s*,?\s*/\*(.*?)\*/", h, re.S)
    assert m, "NSK_OPT_INNER_MATRIX_PRECISION is not declared with a comment in include/nsk.h"
    assert S.OPT_INNER_MATRIX_PRECISION == int(m.group(1)) == 17
    doc = " ".join(m.group(2).split())
    for what in ("64", "32", "inner", "deviation", "NSK_INNER_MATRIX_PRECISION"):
        assert what.lower() in doc.lower(), what


def test_inner_exports_are_declared_and_listed():
    from navier_stokes_solver_amd import solver as S
    h = _header()
    assert re.search(r"int\s+nsk_inner_value_bytes\s*\(\s*nsk_handle\s+h\s*,\s*int\s+blk\s*,\s*int32_t\s*\*\s*bytes\s*\)", h)
    assert re.search(r"int\s+nsk_inner_spmv\s*\(\s*nsk_handle\s+h\s*,\s*int\s+blk\s*,\s*const\s+double\s*\*\s*x_owned\s*,"
                     r"\s*double\s*\*\s*y\s*\)", h)
    for name in ("nsk_inner_value_bytes", "nsk_inner_spmv"):
        assert name in S.EXPORTS, name


def test_out_of_range_error_code_is_listed():
    """The set-up's error for a value that is finite in fp64 and outside fp32's range is in the header's list."""
    h = _header()
    m = re.search(r"^\s*\*\s*-48\b(.*)$", h, re.M)
    assert m and "NSK_OPT_INNER_MATRIX_PRECISION" in m.group(1) and "fp32" in m.group(1)
