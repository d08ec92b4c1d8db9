"""NSK_OPT_INNER_BASIS_PRECISION in the public header, the Python wrapper, the library's source and the documents (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_option_value_matches_the_header_and_is_documented():
    from navier_stokes_solver_amd import solver as S
    h = _read("include", "nsk.h")
    m = re.search(r"NSK_OPT_INNER_BASIS_PRECISION\s*=\s*(\d+)\s*,?\s*/\*(.*?)\*/", h, re.S)
    assert m, "NSK_OPT_INNER_BASIS_PRECISION is not declared with a comment in include/nsk.h"
    assert S.OPT_INNER_BASIS_PRECISION == int(m.group(1)) == 18
    doc = " ".join(m.group(2).split())
    for what in ("64", "32", "inner FGMRES on F", "deviation", "NSK_INNER_BASIS_PRECISION", "-61", "working vector",
                 "NSK_OPT_INNER_FUSED_GS = 0", "NSK_OPT_BLAS1_PAIRS = 0", "nsk_inner_basis_bytes"):
        assert what.lower() in doc.lower(), what
    # the ids of the public options stay distinct
    ids = re.findall(r"^\s*NSK_OPT_\w+\s*=\s*(\d+)", h, re.M)
    assert len(ids) == len(set(ids))


def test_the_getter_is_declared_listed_and_wrapped():
    from navier_stokes_solver_amd import solver as S
    h = _read("include", "nsk.h")
    assert re.search(r"int\s+nsk_inner_basis_bytes\s*\(\s*nsk_handle\s+h\s*,\s*int32_t\s*\*\s*bytes\s*\)", h)
    assert "nsk_inner_basis_bytes" in S.EXPORTS
    assert callable(getattr(S.LinearSolver, "inner_basis_bytes"))


def test_the_environment_override_is_read_once_and_takes_32_or_64_only():
    """The library's own parsing, as for the two other precision options: a function-local static (read once per
    process), atoi, and every value but 32 and 64 counts as unset."""
    csrc = {n: _read("navier_stokes_solver_amd", "csrc", n)
            for n in ("nsk_handle.hpp", "nsk_precond.cpp", "nsk_capi.cpp", "nsk_capi_assembly.cpp", "nsk_debug.cpp")}
    src = csrc["nsk_precond.cpp"]
    m = re.search(r"static const int (\w+) = \[\] \{\s*const char \*e = std::getenv\(\"NSK_INNER_BASIS_PRECISION\"\);"
                  r"\s*const int v = e \? std::atoi\(e\) : 0;\s*return v == 32 \|\| v == 64 \? v : 0;\s*\}\(\);", src)
    assert m, "NSK_INNER_BASIS_PRECISION is not parsed the way NSK_INNER_MATRIX_PRECISION is"
    name = m.group(1)
    assert re.search(rf"\({name} \? {name} : inner_basis_precision\) == 32", src)
    assert "\n".join(csrc.values()).count('getenv("NSK_INNER_BASIS_PRECISION")') == 1
    # the option itself: 64 or 32, anything else is error -61
    assert re.search(r"case NSK_OPT_INNER_BASIS_PRECISION:\s*if \(v != 64\.0 && v != 32\.0\) throw Error\(-61,", csrc["nsk_capi.cpp"])


def test_both_drivers_print_the_line():
    line = "[nsk] NSK_INNER_BASIS_PRECISION=32: inner FGMRES basis on F stored in fp32 (deviation from the reference)"
    assert line in _read("navier_stokes_solver_amd", "csrc", "cli_main.cpp")
    assert line in _read("navier_stokes_solver_amd", "newton.py")


def test_the_documents_name_the_option_the_switch_and_the_getter():
    readme, design = _read("README.md"), _read("DESIGN.md")
    assert "NSK_INNER_BASIS_PRECISION=32|64" in readme and "NSK_OPT_INNER_BASIS_PRECISION" in readme
    m = re.search(r"^## 5l\. .*$", design, re.M)
    assert m and "NSK_OPT_INNER_BASIS_PRECISION" in m.group(0)
    sec = design[m.start():]
    sec = sec[:re.search(r"^## (?!5l)", sec[4:], re.M).start() + 4]
    for what in ("nsk_inner_basis_bytes", "NSK_INNER_BASIS_PRECISION", "working vector", "stays double",
                 "NSK_OPT_INNER_FUSED_GS = 0", "NSK_OPT_BLAS1_PAIRS", "profiles/inner_basis_precision_kernel_resource_usage.txt"):
        assert what in sec, what


def test_the_hook_ops_are_declared():
    ih = _read("navier_stokes_solver_amd", "csrc", "nsk_internal.h")
    for name, val in (("MULTI_DOT_ALL_F32", 16), ("MULTI_AXPY_ALL_F32", 17), ("GS_COLUMN_F32", 18), ("EQU", 19), ("EQU_F32", 20)):
        assert re.search(rf"NSK_DBG_KRY_{name}\s*=\s*{val}\b", ih), name
