"""What a set-up takes of the options and their environment overrides, restated from the rules of include/nsk.h (no GPU),
and the two hooks of nsk_internal.h that run the library's own parsers and resolver on bare values.

The rules (include/nsk.h, the comments of the options; nsk_internal.h for NSK_IOPT_AMG_FUSED_CHEBY):
  * a precision override set to 32 or 64 replaces the option, any other text leaves it; a switch set to exactly "0" or
    "1" replaces the option, any other text leaves it;
  * NSK_OPT_FACTOR_PRECISION, NSK_OPT_INNER_MATRIX_PRECISION, NSK_OPT_INNER_BASIS_PRECISION and
    NSK_OPT_INNER_MATRIX_FREE_F are wanted or not whatever the preconditioner (what the set-up can do with them is not
    the resolver's business: the getters report it);
  * NSK_OPT_VELOCITY_AMG means the stationary blockTriangular set-up only, NSK_OPT_SCHUR_AMG and
    NSK_OPT_ASIMPLE_VELOCITY_AMG the stationary aSIMPLE set-up only;
  * NSK_OPT_AMG_PRECISION = 32 gives a hierarchy 32 bits only where this set-up wants that hierarchy;
  * the fused Chebyshev steps belong to the hierarchy of NSK_OPT_ASIMPLE_VELOCITY_AMG alone, and -1 and 1 both mean on;
  * stationary blockDiagonal applies SSOR (kind 1) to both blocks, everything else ILU (kind 0)."""
import ctypes as C

KNOBS = ("factor_precision", "inner_matrix_precision", "inner_basis_precision", "amg_precision", "matrix_free_f",
         "schur_amg", "asimple_velocity_amg", "amg_fused_cheby", "velocity_amg")
ENV_NAMES = ("NSK_FACTOR_PRECISION", "NSK_INNER_MATRIX_PRECISION", "NSK_INNER_BASIS_PRECISION", "NSK_AMG_PRECISION",
             "NSK_INNER_MATRIX_FREE_F", "NSK_SCHUR_AMG", "NSK_ASIMPLE_VELOCITY_AMG", "NSK_AMG_FUSED_CHEBY")
DEFAULTS = dict(factor_precision=64, inner_matrix_precision=64, inner_basis_precision=64, amg_precision=64, matrix_free_f=0,
                schur_amg=0, asimple_velocity_amg=0, amg_fused_cheby=-1, velocity_amg=1)
# the values nsk_set_option stores for each knob, and what its override parses to (the first: unset)
OPTION_VALUES = dict(factor_precision=(64, 32), inner_matrix_precision=(64, 32), inner_basis_precision=(64, 32),
                     amg_precision=(64, 32), matrix_free_f=(0, 1), schur_amg=(0, 1), asimple_velocity_amg=(0, 1),
                     amg_fused_cheby=(-1, 0, 1), velocity_amg=(0, 1))
ENV_VALUES = {k: (0, 32, 64) if k.endswith("precision") else (-1, 0, 1) for k in KNOBS[:8]}
ENV_UNSET = {k: ENV_VALUES[k][0] for k in KNOBS[:8]}
FIELDS = ("factor32", "amg_bits_F", "want_amgF", "fused_cheby", "want_amgS", "amg_bits_S", "inner32", "matfree", "basis32",
          "kindF", "kindP", "velocity_amg_wanted")
SETUPS = tuple((t, v) for t in (0, 1, 2) for v in (0, 1))   # (type, variant)
PRECISION, SWITCH = 0, 1                                    # nsk_debug_env_parse's kinds
# (text, precision parser, switch parser)
ENV_TEXTS = ((None, 0, -1), ("", 0, -1), ("0", 0, 0), ("1", 0, 1), ("01", 0, -1), ("1 ", 0, -1), ("2", 0, -1), ("yes", 0, -1),
             ("32", 32, -1), ("64", 64, -1), ("16", 0, -1), ("32x", 32, -1), (" 64", 64, -1))


def _lib():
    from navier_stokes_solver_amd import solver as S
    L = S.lib()   # (no GPU call)
    L.nsk_debug_env_parse.argtypes = [C.c_int, C.c_char_p]
    L.nsk_debug_setup_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def env_parse(kind, text):
    return _lib().nsk_debug_env_parse(kind, None if text is None else text.encode())


def library_plan(req, env, type_, variant):
    """The library's resolver on the dicts `req` (nine knobs) and `env` (eight parsed overrides)."""
    r = (C.c_int * 9)(*[req[k] for k in KNOBS])
    e = (C.c_int * 8)(*[env[k] for k in KNOBS[:8]])
    out = (C.c_int * len(FIELDS))()
    assert _lib().nsk_debug_setup_plan(r, e, type_, variant, out) == len(FIELDS)
    return dict(zip(FIELDS, out))


def expected_plan(req, env, type_, variant):
    """The same from the rules above."""
    def taken(k):
        return req[k] if env[k] == ENV_UNSET[k] else env[k]

    block_diagonal, block_triangular, asimple = (type_ == t for t in (0, 1, 2))
    stationary = variant == 0
    velocity_amg = block_triangular and stationary and req["velocity_amg"] == 1
    amg_f = asimple and stationary and taken("asimple_velocity_amg") == 1
    amg_s = asimple and stationary and taken("schur_amg") == 1
    fp32_cycles = taken("amg_precision") == 32
    ssor = 1 if block_diagonal and stationary else 0
    return dict(factor32=int(taken("factor_precision") == 32),
                amg_bits_F=32 if fp32_cycles and (velocity_amg or amg_f) else 64,
                want_amgF=int(amg_f),
                fused_cheby=int(amg_f and taken("amg_fused_cheby") in (-1, 1)),
                want_amgS=int(amg_s),
                amg_bits_S=32 if fp32_cycles and amg_s else 64,
                inner32=int(taken("inner_matrix_precision") == 32),
                matfree=int(taken("matrix_free_f") == 1),
                basis32=int(taken("inner_basis_precision") == 32),
                kindF=ssor, kindP=ssor,
                velocity_amg_wanted=int(velocity_amg))


def check_knob(knob, setups=SETUPS):
    """Every (option value, environment value) pair of one knob over the given set-ups, the others at their defaults:
    the library's resolver against the rules.  Returns the number of cases."""
    n = 0
    for opt in OPTION_VALUES[knob]:
        for ev in ENV_VALUES.get(knob, (None,)):
            req, env = dict(DEFAULTS, **{knob: opt}), dict(ENV_UNSET)
            if ev is not None:
                env[knob] = ev
            for t, v in setups:
                got, want = library_plan(req, env, t, v), expected_plan(req, env, t, v)
                assert got == want, (knob, opt, ev, t, v, got, want)
                n += 1
    return n
