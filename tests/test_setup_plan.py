"""The resolver of the preconditioner set-up (resolve_setup, csrc/nsk_handle.hpp) through nsk_debug_setup_plan, against the
rules of include/nsk.h as tests/setup_plan_reference.py restates them (no GPU: no handle, no device, no environment)."""
import itertools
import os
import re

import pytest

from tests import setup_plan_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_defaults_are_the_ones_the_public_header_names():
    h = open(os.path.join(ROOT, "include", "nsk.h")).read()
    ih = open(os.path.join(ROOT, "navier_stokes_solver_amd", "csrc", "nsk_internal.h")).read()
    for opt, default in (("FACTOR_PRECISION", "64"), ("INNER_MATRIX_PRECISION", "64"), ("INNER_BASIS_PRECISION", "64"),
                         ("AMG_PRECISION", "64"), ("INNER_MATRIX_FREE_F", "0"), ("SCHUR_AMG", "0"),
                         ("ASIMPLE_VELOCITY_AMG", "0"), ("VELOCITY_AMG", "1")):
        m = re.search(rf"NSK_OPT_{opt}\s*=\s*\d+\s*,?\s*/\*(.*?)\*/", h, re.S)
        assert m and f"{default} (default)" in " ".join(m.group(1).split()), opt
        assert R.DEFAULTS["matrix_free_f" if opt == "INNER_MATRIX_FREE_F" else opt.lower()] == int(default)
    assert re.search(r"NSK_IOPT_AMG_FUSED_CHEBY = 113, // -1 \(default\)", ih) and R.DEFAULTS["amg_fused_cheby"] == -1
    # with everything at its default and nothing in the environment: what the reference configures
    for t, v in R.SETUPS:
        p = R.library_plan(R.DEFAULTS, R.ENV_UNSET, t, v)
        assert p == R.expected_plan(R.DEFAULTS, R.ENV_UNSET, t, v)
        assert p == dict(factor32=0, amg_bits_F=64, want_amgF=0, fused_cheby=0, want_amgS=0, amg_bits_S=64, inner32=0,
                         matfree=0, basis32=0, kindF=int((t, v) == (0, 0)), kindP=int((t, v) == (0, 0)),
                         velocity_amg_wanted=int((t, v) == (1, 0)))


@pytest.mark.parametrize("knob", R.KNOBS)
def test_every_option_and_override_value_of_one_knob_over_all_set_ups(knob):
    n_env = len(R.ENV_VALUES.get(knob, (None,)))
    assert R.check_knob(knob) == len(R.OPTION_VALUES[knob]) * n_env * 6


def test_an_override_that_is_set_wins_and_one_that_is_unset_leaves_the_option():
    """Stated on the resolved fields directly (not through the restatement), in the set-up where each knob acts."""
    acts = dict(factor_precision=("factor32", (0, 1), 32), inner_matrix_precision=("inner32", (1, 1), 32),
                inner_basis_precision=("basis32", (2, 0), 32), amg_precision=("amg_bits_F", (1, 0), 32),
                matrix_free_f=("matfree", (1, 0), 1), schur_amg=("want_amgS", (2, 0), 1),
                asimple_velocity_amg=("want_amgF", (2, 0), 1))
    for knob, (field, (t, v), on) in acts.items():
        for opt in R.OPTION_VALUES[knob]:
            for ev in R.ENV_VALUES[knob]:
                got = R.library_plan(dict(R.DEFAULTS, **{knob: opt}), dict(R.ENV_UNSET, **{knob: ev}), t, v)[field]
                taken = opt if ev == R.ENV_UNSET[knob] else ev
                assert got == ((32 if taken == on else 64) if field == "amg_bits_F" else int(taken == on)), (knob, opt, ev)


@pytest.mark.parametrize("env_amg", R.ENV_VALUES["amg_precision"])
def test_amg_precision_32_reaches_a_hierarchy_only_where_the_set_up_wants_it(env_amg):
    for vel, asimple, schur in itertools.product((0, 1), repeat=3):
        req = dict(R.DEFAULTS, amg_precision=32, velocity_amg=vel, asimple_velocity_amg=asimple, schur_amg=schur)
        env = dict(R.ENV_UNSET, amg_precision=env_amg)
        bits = 64 if env_amg == 64 else 32
        for t, v in R.SETUPS:
            p = R.library_plan(req, env, t, v)
            assert p == R.expected_plan(req, env, t, v), (vel, asimple, schur, t, v)
            want_f = ((t, v) == (1, 0) and vel) or ((t, v) == (2, 0) and asimple)
            assert p["amg_bits_F"] == (bits if want_f else 64)
            assert p["amg_bits_S"] == (bits if (t, v) == (2, 0) and schur else 64)
            assert p["want_amgF"] == int((t, v) == (2, 0) and asimple) and p["want_amgS"] == int((t, v) == (2, 0) and schur)
            assert p["velocity_amg_wanted"] == int((t, v) == (1, 0) and vel)


def test_the_fused_smoother_steps_follow_the_velocity_hierarchy_of_asimple_and_minus_one_counts_as_on():
    for opt, ev, asimple in itertools.product((-1, 0, 1), (-1, 0, 1), (0, 1)):
        req, env = dict(R.DEFAULTS, amg_fused_cheby=opt, asimple_velocity_amg=asimple), dict(R.ENV_UNSET, amg_fused_cheby=ev)
        for t, v in R.SETUPS:
            p = R.library_plan(req, env, t, v)
            on = (opt != 0) if ev == -1 else ev == 1
            assert p["fused_cheby"] == int(on and asimple == 1 and (t, v) == (2, 0)), (opt, ev, asimple, t, v)
            assert p == R.expected_plan(req, env, t, v)
    # the override of the hierarchy itself switches them with it
    for ev, want in ((1, 1), (0, 0)):
        p = R.library_plan(dict(R.DEFAULTS, asimple_velocity_amg=1 - ev), dict(R.ENV_UNSET, asimple_velocity_amg=ev), 2, 0)
        assert (p["want_amgF"], p["fused_cheby"]) == (want, want)
