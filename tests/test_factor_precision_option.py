"""NSK_OPT_FACTOR_PRECISION in the public header and in the Python wrapper (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "nsk.h")) as f:
        return f.read()


def test_option_value_matches_the_header_and_is_documented():
    from navier_stokes_solver_amd import solver as S
    h = _header()
    m = re.search(r"NSK_OPT_FACTOR_PRECISION\s*=\s*(\d+)\s*,?\s*/\*(.*?)\*/", h, re.S)
    assert m, "NSK_OPT_FACTOR_PRECISION is not declared with a comment in include/nsk.h"
    assert S.OPT_FACTOR_PRECISION == int(m.group(1)) == 16
    doc = " ".join(m.group(2).split())
    for what in ("64", "32", "off-diagonal", "deviation", "NSK_FACTOR_PRECISION"):
        assert what.lower() in doc.lower(), what


def test_value_bytes_getter_is_declared_and_exported():
    from navier_stokes_solver_amd import solver as S
    assert re.search(r"int\s+nsk_tri_get_value_bytes\s*\(\s*nsk_handle\s+h\s*,\s*int\s+which\s*,\s*int32_t\s*\*\s*bytes\s*\)",
                     _header())
    assert "nsk_tri_get_value_bytes" in S.EXPORTS
