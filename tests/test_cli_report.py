"""The drivers' report from the device-resident solution: the C++ drivers write the VTU record and print the
coefficients the Python drivers print; the Python drivers' device report against their host report
(NSK_HOST_POSTPROCESS=1) and on two ranks against one."""
import filecmp
import io
import os
import re
import subprocess
import xml.etree.ElementTree as ET
from contextlib import redirect_stdout

import numpy as np
import pytest

from navier_stokes_solver_amd import cli

pytestmark = pytest.mark.gpu

ARGS = ["-m", "16,10", "-r", "30", "-s", "1", "-p", "2", "-t", "1e-11"]      # levels 10 and 30: Stokes and Newton phase
# the comparisons between two Python runs: the first level alone (the inlet ramp of the Stokes phase) — a third of the
# solves, the same report
FIRST_LEVEL = ["-m", "16,10", "-r", "10", "-s", "1", "-p", "2", "-t", "1e-10"]


def _bin(name):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navier_stokes_solver_amd", "bin", name)


def _coefficients(text):
    num = r" (-?[0-9.]+(?:e[+-]?[0-9]+)?)\n"
    return re.findall(r"Lift coefficient:" + num, text), re.findall(r"Drag coefficient:" + num, text)


def _point_data(path):
    piece = ET.parse(path).getroot().find("UnstructuredGrid/Piece")
    arrays = {a.get("Name"): np.array(a.text.split(), float) for a in piece.find("PointData")}
    pts = np.array(piece.find("Points/DataArray").text.split(), float).reshape(-1, 3)
    return int(piece.get("NumberOfCells")), int(piece.get("NumberOfPoints")), pts, arrays


@pytest.fixture(scope="module")
def python_runs(tmp_path_factory):
    """The Python driver's runs, once for the module: ARGS with the device report; FIRST_LEVEL with the device report, the
    host report and on two ranks."""
    runs = {}
    for key, args, env in (("full", ARGS, {}), ("device", FIRST_LEVEL, {}), ("host", FIRST_LEVEL, {"NSK_HOST_POSTPROCESS": "1"}),
                           ("ranks2", FIRST_LEVEL, {"NSK_RANKS": "2"})):
        d = tmp_path_factory.mktemp(key)
        mp = pytest.MonkeyPatch()
        try:
            mp.setenv("NSK_OUTPUT_DIR", str(d))
            mp.delenv("NSK_HOST_POSTPROCESS", raising=False)
            mp.delenv("NSK_RANKS", raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            out = io.StringIO()
            with redirect_stdout(out):
                assert cli.main(["StationaryNSSolver"] + args) == 0
        finally:
            mp.undo()
        runs[key] = (d, out.getvalue())
    return runs


def test_cpp_stationary_driver_reports_like_the_python_driver(tmp_path, python_runs):
    env = dict(os.environ, NSK_OUTPUT_DIR=str(tmp_path))
    cpp = subprocess.run([_bin("StationaryNSSolver")] + ARGS, capture_output=True, text=True, timeout=300, env=env)
    assert cpp.returncode == 0, cpp.stderr
    vtu, pvtu = tmp_path / "output-stokes_0.0.vtu", tmp_path / "output-stokes_0.pvtu"
    assert vtu.exists() and pvtu.exists() and sorted(os.listdir(tmp_path)) == ["output-stokes_0.0.vtu", "output-stokes_0.pvtu"]
    n_cells, n_pts, pts, arrays = _point_data(vtu)
    assert (n_cells, n_pts) == (158, 632) and set(arrays) == {"velocity", "pressure", "partitioning"}
    assert ET.parse(pvtu).getroot().find("PUnstructuredGrid/Piece").get("Source") == "output-stokes_0.0.vtu"
    lift, drag = _coefficients(cpp.stdout)
    assert len(lift) == 1 and len(drag) == 1
    for line in ("Output written to output-stokes", "Computing lift and drag forces"):
        assert cpp.stdout.count(line) == 1
    # against the Python driver's run of the same command: the margin test_cpp_and_python_newton_drivers_agree allows
    # between the two drivers' residuals
    d, text = python_runs["full"]
    assert filecmp.cmp(pvtu, d / "output-stokes_0.pvtu", shallow=False)
    plift, pdrag = _coefficients(text)
    assert len(plift) == 1 and len(pdrag) == 1
    scale = abs(float(pdrag[0]))
    assert abs(float(drag[0]) - float(pdrag[0])) <= 1e-5 * scale and abs(float(lift[0]) - float(plift[0])) <= 1e-5 * scale
    n2, m2, pts2, arrays2 = _point_data(d / "output-stokes_0.0.vtu")
    assert (n2, m2) == (n_cells, n_pts) and np.array_equal(pts, pts2)
    for k in ("velocity", "pressure", "partitioning"):
        assert np.abs(arrays[k] - arrays2[k]).max() <= 1e-5 * np.abs(arrays2[k]).max(), k
    assert np.abs(arrays["velocity"]).max() > 0 and np.all(arrays["partitioning"] == 0.0)


def test_cpp_unsteady_driver_reports_every_step(tmp_path):
    env = dict(os.environ, NSK_OUTPUT_DIR=str(tmp_path))
    out = subprocess.run([_bin("NSSolver"), "-T", "0.02,0.01", "-m", "16,10", "-r", "11", "-s", "1", "-p", "2", "-t", "1e-8"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert sorted(os.listdir(tmp_path)) == ["output_001.0.vtu", "output_001.pvtu", "output_002.0.vtu", "output_002.pvtu"]
    lift, drag = _coefficients(out.stdout)
    assert len(lift) == 2 and len(drag) == 2
    for step in (1, 2):
        n_cells, n_pts, _, arrays = _point_data(tmp_path / f"output_00{step}.0.vtu")
        assert (n_cells, n_pts) == (158, 632) and np.isfinite(arrays["velocity"]).all()
    # each record follows its step's Newton solve
    assert out.stdout.index("n =   1") < out.stdout.index("Drag coefficient:") < out.stdout.index("n =   2")


def test_device_report_is_the_host_report(python_runs):
    """The same command with and without NSK_HOST_POSTPROCESS=1: equal VTU files, the same drag text, every other line
    of the output equal (the lift line: next test)."""
    (d0, t0), (d1, t1) = python_runs["device"], python_runs["host"]
    assert _coefficients(t0)[1] == _coefficients(t1)[1] and len(_coefficients(t0)[1]) == 1
    files = sorted(os.listdir(d1))
    assert files == ["output-stokes_0.0.vtu", "output-stokes_0.pvtu"] == sorted(os.listdir(d0))
    assert filecmp.cmpfiles(d0, d1, files, shallow=False) == (files, [], [])
    strip = lambda t: [ln for ln in t.splitlines() if not ln.startswith(("[nsk]", "Lift coefficient:"))]   # noqa: E731
    assert strip(t0) == strip(t1) and t0.count("Lift coefficient:") == 1      # ([nsk]: the timing line)


def test_device_report_prints_the_host_reports_lift_text(python_runs):
    """The lift coefficient as text, device report against host report, on FIRST_LEVEL.

    Nothing but the order of two sums decides this text: the generated mesh is symmetric about y = 0.205 and so is the
    stationary flow, the lift force is what cancellation leaves of terms of size A ~ 1, and `postprocess.lift_drag`
    adds its terms in numpy's order, `nsk_forces` in the fixed order of its slots.  On the first level the two texts are
    equal on an MI355X.  With `-m 16,10 -r 30 -s 1 -p 2 -t 1e-11` (ARGS) they are not: device `Lift coefficient:
    3.03676e-11`, host `Lift coefficient: 3.03665e-11`, both next to `Drag coefficient: 3.94346` — 1.1e-15 apart in the
    coefficient, 2.4e-17 in the force, far inside the rounding bound both integrals obey (tests/test_gpu_forces.py)."""
    t0, t1 = python_runs["device"][1], python_runs["host"][1]
    print("device:", _coefficients(t0), "host:", _coefficients(t1))
    assert _coefficients(t0)[0] == _coefficients(t1)[0] and len(_coefficients(t0)[0]) == 1


def test_two_ranks_report_the_one_rank_coefficients(python_runs):
    (_, t1), (d2, t2) = python_runs["device"], python_runs["ranks2"]
    (l1, c1), (l2, c2) = _coefficients(t1), _coefficients(t2)
    assert len(l2) == 1 and len(c2) == 1
    scale = abs(float(c1[0]))
    assert abs(float(c1[0]) - float(c2[0])) <= 1e-6 * scale and abs(float(l1[0]) - float(l2[0])) <= 1e-6 * scale
    assert sorted(os.listdir(d2)) == ["output-stokes_0.0.vtu", "output-stokes_0.1.vtu", "output-stokes_0.pvtu"]
    cells = [_point_data(d2 / f"output-stokes_0.{r}.vtu") for r in range(2)]
    assert cells[0][0] + cells[1][0] == 158 and np.all(cells[1][3]["partitioning"] == 1.0)
