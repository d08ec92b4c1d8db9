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
    """The library's own parsing, as for the other precision options: one function-local static (read once per process)
    holds all eight overrides, atoi, and every value but 32 and 64 counts as unset."""
    from tests import setup_plan_reference as R
    csrc = {n: _read("navier_stokes_solver_amd", "csrc", n)
            for n in ("nsk_handle.hpp", "nsk_precond.cpp", "nsk_capi.cpp", "nsk_capi_assembly.cpp", "nsk_debug.cpp")}
    # read once, in one place: one getenv per override across the handle files, all inside the one static
    m = re.search(r"inline const SetupEnv &setup_env\(\) \{\s*static const SetupEnv env = \{(.*?)\};\s*return env;\s*\}",
                  csrc["nsk_handle.hpp"], re.S)
    assert m, "the overrides are not read by one function-local static behind one accessor"
    for name in R.ENV_NAMES:
        assert "\n".join(csrc.values()).count(f'getenv("{name}")') == 1, name
        kind = "precision" if name.endswith("PRECISION") else "switch"
        assert f'parse_env_{kind}(std::getenv("{name}"))' in m.group(1), name
    # accepts only these values
    for text, precision, _ in R.ENV_TEXTS:
        assert R.env_parse(R.PRECISION, text) == precision, text
    # the override wins over the option, and unset leaves the option: every pair, in every set-up
    for opt in (64, 32):
        for env in (0, 32, 64):
            for t, v in R.SETUPS:
                plan = R.library_plan(dict(R.DEFAULTS, inner_basis_precision=opt), dict(R.ENV_UNSET, inner_basis_precision=env), t, v)
                assert plan["basis32"] == int((env if env else opt) == 32), (opt, env, t, v)
    assert re.search(r"basis32_wanted = plan\.basis32;", csrc["nsk_precond.cpp"])
    # the option itself: 64 or 32, anything else is error -61 (the helper of the plain cases throws it)
    assert re.search(r"case NSK_OPT_INNER_BASIS_PRECISION:\s*req\.inner_basis_precision = one_of\(v, \{64, 32\}, "
                     r"\"NSK_OPT_INNER_BASIS_PRECISION: 64 or 32\"\);", csrc["nsk_capi.cpp"])
    assert re.search(r"static int one_of\(double v, std::initializer_list<double> allowed, const char \*text\) \{\s*"
                     r"for \(const double a : allowed\)\s*if \(v == a\) return \(int\)v;\s*throw Error\(-61, text\);\s*\}",
                     csrc["nsk_capi.cpp"])


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
