"""The drivers with NSK_VTU_FORMAT=binary: the record as raw appended data from `nsk_state_get_record`, read back
by tests/vtu_record_reader.py and held against the ASCII record of the same command — the Python drivers on one and two
ranks, with subdivided patches and on a gmsh mesh, and both C++ drivers."""
import io
import os
import subprocess
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest

from navier_stokes_solver_amd import cli
from tests import vtu_record_reader as VR
from tests.test_cli_report import FIRST_LEVEL, _bin, _coefficients
from tests.test_simplex import REF_MESH

pytestmark = pytest.mark.gpu

SWITCHES = ("NSK_VTU_FORMAT", "NSK_VTU_SUBDIVISIONS", "NSK_HOST_POSTPROCESS", "NSK_RANKS")
UNSTEADY = ["-T", "0.02,0.01", "-m", "16,10", "-r", "11", "-s", "1", "-p", "2", "-t", "1e-8"]


def _python_run(d, args, env):
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("NSK_OUTPUT_DIR", str(d))
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            rc = cli.main(["StationaryNSSolver"] + args)
    finally:
        mp.undo()
    return rc, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def python_runs(tmp_path_factory):
    """The Python driver on FIRST_LEVEL, once for the module: ASCII, binary, binary with 3 x 3 patches, binary on two ranks."""
    runs = {}
    for key, env in (("ascii", {}), ("binary", {"NSK_VTU_FORMAT": "binary"}),
                     ("s3", {"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "3"}),
                     ("ranks2", {"NSK_VTU_FORMAT": "binary", "NSK_RANKS": "2"})):
        d = tmp_path_factory.mktemp(key)
        rc, out, err = _python_run(d, FIRST_LEVEL, env)
        assert rc == 0, err
        runs[key] = (d, out)
    return runs


def _without_nsk_lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith("[nsk]")]


def _same_tokens(binary, ascii_, fmt="%.12g"):
    """Every value of the binary file prints as the token of the ASCII file."""
    assert (binary["n_points"], binary["n_cells"]) == (ascii_["n_points"], ascii_["n_cells"])
    assert binary["point_data"] == ascii_["point_data"] and binary["types"] == ascii_["types"]
    for name in ("velocity", "pressure"):
        assert [fmt % v for v in binary["arrays"][name].reshape(-1)] == ascii_["tokens"][name], name
    assert [fmt % v for v in binary["arrays"]["points"].reshape(-1)] == ascii_["point_tokens"]
    for name in ("connectivity", "offsets", "types"):
        assert np.array_equal(binary["arrays"][name], ascii_["arrays"][name]), name
    if "partitioning" in ascii_["arrays"]:
        assert np.array_equal(binary["arrays"]["partitioning"], ascii_["arrays"]["partitioning"])
    assert np.abs(binary["arrays"]["velocity"]).max() > 0


def test_binary_record_of_the_python_driver_is_the_ascii_record(python_runs):
    (d0, t0), (d1, t1) = python_runs["ascii"], python_runs["binary"]
    assert _without_nsk_lines(t0) == _without_nsk_lines(t1)
    assert sum(ln.startswith("[nsk] NSK_VTU_FORMAT=binary") for ln in t1.splitlines()) == 1 and "NSK_VTU_FORMAT" not in t0
    files = ["output-stokes_0.0.vtu", "output-stokes_0.pvtu"]
    assert sorted(os.listdir(d0)) == files == sorted(os.listdir(d1))
    assert (d0 / files[1]).read_bytes() == (d1 / files[1]).read_bytes()
    got, txt = VR.read(d1 / files[0]), VR.read(d0 / files[0])
    VR.check_layout(got)
    assert (got["n_points"], got["n_cells"]) == (632, 158)
    _same_tokens(got, txt)


def test_subdivided_patches_carry_the_vertex_values(python_runs):
    (d1, _), (d3, t3) = python_runs["binary"], python_runs["s3"]
    assert sorted(os.listdir(d3)) == ["output-stokes_0.0.vtu", "output-stokes_0.pvtu"]
    assert _coefficients(t3) == _coefficients(python_runs["binary"][1])
    assert any(ln.startswith("[nsk] NSK_VTU_FORMAT=binary") and "3 x 3" in ln for ln in t3.splitlines())
    one, sub = VR.read(d1 / "output-stokes_0.0.vtu"), VR.read(d3 / "output-stokes_0.0.vtu")
    VR.check_layout(sub)
    assert (sub["n_points"], sub["n_cells"]) == (158 * 16, 158 * 9)
    corners = [0, 3, 12, 15]                                         # pt = l * 4 + k with k, l in {0, 3}
    for name, nc in (("points", 3), ("velocity", 3), ("pressure", 1), ("partitioning", 1)):
        a = sub["arrays"][name].reshape(158, 16, nc)[:, corners]
        assert a.tobytes() == one["arrays"][name].reshape(158, 4, nc).tobytes(), name
    assert np.isfinite(sub["arrays"]["velocity"]).all() and np.all(sub["arrays"]["types"] == 9)
    # the nine quads of a cell tile it: every point of the cell is used, the corners once, the inner points four times
    conn = sub["arrays"]["connectivity"].reshape(158, 36)
    assert np.array_equal(np.bincount(conn[5] - 5 * 16, minlength=16), [1, 2, 2, 1, 2, 4, 4, 2, 2, 4, 4, 2, 1, 2, 2, 1])


def test_binary_record_on_two_ranks(python_runs):
    (d1, t1), (d2, t2) = python_runs["binary"], python_runs["ranks2"]
    assert sorted(os.listdir(d2)) == ["output-stokes_0.0.vtu", "output-stokes_0.1.vtu", "output-stokes_0.pvtu"]
    pieces = [VR.read(d2 / f"output-stokes_0.{r}.vtu") for r in range(2)]
    for r, p in enumerate(pieces):
        VR.check_layout(p)
        assert np.all(p["arrays"]["partitioning"] == float(r)) and p["n_points"] == 4 * p["n_cells"]
        assert np.isfinite(p["arrays"]["velocity"]).all()
    assert pieces[0]["n_cells"] + pieces[1]["n_cells"] == 158
    assert b'Source="output-stokes_0.1.vtu"' in (d2 / "output-stokes_0.pvtu").read_bytes()
    # the pieces side by side are the cells of the one-rank record, in its order (x-strips, cells in (i, j) order)
    one = VR.read(d1 / "output-stokes_0.0.vtu")
    assert np.array_equal(np.concatenate([p["arrays"]["points"] for p in pieces]), one["arrays"]["points"])
    (l1, c1), (l2, c2) = _coefficients(t1), _coefficients(t2)
    assert len(c2) == 1 and abs(float(c1[0]) - float(c2[0])) <= 1e-6 * abs(float(c1[0]))


def _cpp(name, args, d, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env, NSK_OUTPUT_DIR=str(d))
    return subprocess.run([_bin(name)] + args, capture_output=True, text=True, timeout=300, env=e)


def test_binary_record_of_the_cpp_stationary_driver_is_its_ascii_record(tmp_path):
    d0, d1 = tmp_path / "ascii", tmp_path / "binary"
    a, b = _cpp("StationaryNSSolver", FIRST_LEVEL, d0), _cpp("StationaryNSSolver", FIRST_LEVEL, d1, NSK_VTU_FORMAT="binary")
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    strip = lambda t: [ln for ln in t.splitlines() if not ln.startswith("[nsk]")]   # noqa: E731
    assert strip(a.stdout) == strip(b.stdout)
    assert sum(ln.startswith("[nsk] NSK_VTU_FORMAT=binary") for ln in b.stdout.splitlines()) == 1
    files = ["output-stokes_0.0.vtu", "output-stokes_0.pvtu"]
    assert sorted(os.listdir(d0)) == files == sorted(os.listdir(d1))
    assert (d0 / files[1]).read_bytes() == (d1 / files[1]).read_bytes()
    got, txt = VR.read(d1 / files[0]), VR.read(d0 / files[0])
    VR.check_layout(got)
    assert (got["n_points"], got["n_cells"]) == (632, 158)
    _same_tokens(got, txt)


def test_binary_records_of_the_cpp_unsteady_driver(tmp_path):
    out = _cpp("NSSolver", UNSTEADY, tmp_path, NSK_VTU_FORMAT="binary")
    assert out.returncode == 0, out.stderr
    lift, drag = _coefficients(out.stdout)
    files = sorted(os.listdir(tmp_path))
    pieces = [f for f in files if f.endswith(".0.vtu")]
    # one record per time step, counters from 001 (this command takes the two steps test_cli_report.py counts)
    assert len(pieces) == len(drag) == len(lift) >= 2 and pieces[:2] == ["output_001.0.vtu", "output_002.0.vtu"]
    assert files == sorted(pieces + [f.replace(".0.vtu", ".pvtu") for f in pieces])
    for f in pieces:
        rec = VR.read(tmp_path / f)
        VR.check_layout(rec)
        assert (rec["n_points"], rec["n_cells"]) == (632, 158)
        assert np.isfinite(rec["arrays"]["velocity"]).all() and np.isfinite(rec["arrays"]["pressure"]).all()
        assert np.abs(rec["arrays"]["velocity"]).max() > 0


def test_binary_record_of_a_gmsh_mesh_is_its_ascii_record(tmp_path):
    """`StationaryNSSolver -M` on the coarse fixture, one rank, device assembly: the values come from `nsk_state_get_record`."""
    args = ["-M", REF_MESH, "-r", "10", "-s", "1", "-p", "2", "-t", "1e-10"]
    d0, d1 = tmp_path / "ascii", tmp_path / "binary"
    os.makedirs(d0), os.makedirs(d1)
    (rc0, t0, e0), (rc1, t1, e1) = _python_run(d0, args, {}), _python_run(d1, args, {"NSK_VTU_FORMAT": "binary"})
    assert rc0 == 0 and rc1 == 0, (e0, e1)
    assert _without_nsk_lines(t0) == _without_nsk_lines(t1)
    assert os.listdir(d0) == ["output-stokes_0.vtu"] == os.listdir(d1)
    got, txt = VR.read(d1 / "output-stokes_0.vtu"), VR.read(d0 / "output-stokes_0.vtu")
    VR.check_layout(got, partitioning=False)
    assert got["n_cells"] == 122 and np.all(got["arrays"]["types"] == 5)
    _same_tokens(got, txt, fmt="%.16g")


def test_rejected_combinations_end_both_driver_families(tmp_path):
    rc, out, err = _python_run(tmp_path, FIRST_LEVEL, {"NSK_VTU_FORMAT": "binary", "NSK_HOST_POSTPROCESS": "1"})
    assert rc != 0 and out == "" and err == "Error: NSK_VTU_FORMAT=binary does not go with NSK_HOST_POSTPROCESS=1\n"
    cpp = _cpp("StationaryNSSolver", FIRST_LEVEL, tmp_path, NSK_VTU_SUBDIVISIONS="3")
    assert cpp.returncode != 0 and cpp.stdout == "" and cpp.stderr == "Error: NSK_VTU_SUBDIVISIONS=3 needs NSK_VTU_FORMAT=binary\n"
    cpp = _cpp("NSSolver", UNSTEADY, tmp_path, NSK_VTU_FORMAT="vtk")
    assert cpp.returncode != 0 and cpp.stdout == "" and "NSK_VTU_FORMAT=vtk" in cpp.stderr
    assert os.listdir(tmp_path) == []
