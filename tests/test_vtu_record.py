"""Host side of the binary VTU record: the appended-raw writers of Python and C++ read back by a reader written
from the rules of the format (tests/vtu_record_reader.py) and held against the ASCII writer, the tables of the subdivided
patches, the drivers' switches, and the extended-precision statement of the s > 1 sums.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from navier_stokes_solver_amd import cli
from navier_stokes_solver_amd import postprocess as PP
from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import simplex as SX
from navier_stokes_solver_amd import gmsh as G
from tests import record_reference as RR
from tests import vtu_record_reader as VR
from tests.forces_reference import local_state
from tests.test_forces_reference import _awkward_state, _patches
from tests.test_simplex import REF_MESH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _strip(nx, ny, lx=PP.LX, nranks=1, rank=0):
    pr = P.generate(nx, ny, nu=0.1, nranks=nranks, rank=rank, lx=lx)
    return pr, np.ascontiguousarray(pr.cell_ij[pr.cell_in_strip != 0], np.int32)


def _want_geometry(ij, hx, hy, s):
    """Points and connectivity by the rule of the issue, cell by cell in plain loops."""
    pts, conn = [], []
    for c, (i, j) in enumerate(ij):
        base = c * (s + 1) ** 2
        for l in range(s + 1):
            for k in range(s + 1):
                pts.append(((i + k / s) * hx, (j + l / s) * hy, 0.0))
        for l in range(s):
            for k in range(s):
                f = base + l * (s + 1) + k
                conn += [f, f + 1, f + (s + 1) + 1, f + (s + 1)]
    return np.array(pts).reshape(-1, 3), np.array(conn, np.int32)


# ---- round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,rank", [(1, 0), (3, 1)])
def test_round_trip_at_one_patch_per_cell_against_the_ascii_writer(tmp_path, nranks, rank):
    nx, ny = 16, 10
    L = PP.Lattice(nx, ny)
    u, p = _awkward_state(L)
    _, ij = _strip(nx, ny, nranks=nranks, rank=rank)
    vel, prs = _patches(L, ij, u, p)
    hx, hy = PP.LX / nx, PP.LY / ny
    rec = PP.VtuRecord.quads(ij, hx, hy, 1, rank)
    rec.vel3[:, :2], rec.prs[:] = vel.reshape(-1, 2), prs.reshape(-1)
    a, b = tmp_path / "bin", tmp_path / "txt"
    f1 = PP.write_vtu_record(rec, str(a), "output", 7, n_digits=3, rank=rank, nranks=nranks)
    f0 = PP.write_vtu_patches(str(b), "output", 7, ij, hx, hy, vel, prs, n_digits=3, rank=rank, nranks=nranks)
    assert os.path.basename(f0) == os.path.basename(f1) and sorted(os.listdir(a)) == sorted(os.listdir(b))
    got, txt = VR.read(f1), VR.read(f0)
    VR.check_layout(got)
    assert os.path.getsize(f1) == got["layout"]["size"] == len(rec.image)
    assert (got["n_points"], got["n_cells"]) == (4 * len(ij), len(ij)) == (txt["n_points"], txt["n_cells"])
    assert got["point_data"] == txt["point_data"] == {"Scalars": "scalars"} and got["types"] == txt["types"]
    # the inputs, exactly
    assert got["arrays"]["velocity"][:, :2].tobytes() == np.ascontiguousarray(vel.reshape(-1, 2)).tobytes()
    assert got["arrays"]["velocity"][:, 2].tobytes() == np.zeros(4 * len(ij)).tobytes()            # the bits of +0.0
    assert got["arrays"]["pressure"].tobytes() == np.ascontiguousarray(prs.reshape(-1)).tobytes()
    assert np.all(got["arrays"]["partitioning"] == float(rank))
    pts, conn = _want_geometry(ij, hx, hy, 1)
    assert np.array_equal(got["arrays"]["points"], pts) and np.array_equal(got["arrays"]["connectivity"], conn)
    # every value prints as the token of the ASCII file
    for name in ("velocity", "pressure", "partitioning"):
        tokens = ["%.12g" % v for v in got["arrays"][name].reshape(-1)]
        if name == "partitioning":
            tokens = [str(float(t)) for t in tokens]                                               # (written as `1.0`)
        assert tokens == txt["tokens"][name], name
    for name in ("connectivity", "offsets", "types"):
        assert np.array_equal(got["arrays"][name], txt["arrays"][name]), name
    assert ["%.12g" % v for v in got["arrays"]["points"].reshape(-1)] == txt["point_tokens"]
    # the record naming the pieces: the ASCII run's, byte for byte
    if rank == 0:
        assert (a / "output_007.pvtu").read_bytes() == (b / "output_007.pvtu").read_bytes()
    else:
        assert not (a / "output_007.pvtu").exists()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_round_trip_of_subdivided_patches(tmp_path, s):
    nx, ny = 16, 10
    _, ij = _strip(nx, ny)
    hx, hy = PP.LX / nx, PP.LY / ny
    rec = PP.VtuRecord.quads(ij, hx, hy, s, 0)
    n = len(ij) * (s + 1) ** 2
    rng = np.random.default_rng(s)
    vel3, prs = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-14, 7, (n, 3)), rng.standard_normal(n)
    vel3[:, 2] = 0.0
    assert rec.vel3.shape == (n, 3) and rec.prs.shape == (n,) and rec.n_points == n and rec.n_cells == len(ij) * s * s
    rec.vel3[:], rec.prs[:] = vel3, prs
    got = VR.read(PP.write_vtu_record(rec, str(tmp_path), "output-stokes", 0))
    VR.check_layout(got)
    assert (got["n_points"], got["n_cells"]) == (n, len(ij) * s * s)
    assert got["arrays"]["velocity"].tobytes() == vel3.tobytes() and got["arrays"]["pressure"].tobytes() == prs.tobytes()
    pts, conn = _want_geometry(ij, hx, hy, s)
    assert np.array_equal(got["arrays"]["points"], pts) and np.array_equal(got["arrays"]["connectivity"], conn)
    assert np.array_equal(got["arrays"]["offsets"], 4 * np.arange(1, len(ij) * s * s + 1))
    assert np.all(got["arrays"]["types"] == 9) and np.all(got["arrays"]["partitioning"] == 0.0)


def test_an_empty_piece_and_bad_subdivisions(tmp_path):
    rec = PP.VtuRecord.quads(np.zeros((0, 2), np.int32), 0.1, 0.1, 3, 2)
    got = VR.read(PP.write_vtu_record(rec, str(tmp_path), "output", 1, rank=2, nranks=3))
    VR.check_layout(got)
    assert (got["n_points"], got["n_cells"]) == (0, 0) and sorted(os.listdir(tmp_path)) == ["output_1.2.vtu"]
    for s in (0, 5):
        with pytest.raises(ValueError):
            PP.VtuRecord.quads(np.zeros((1, 2), np.int32), 0.1, 0.1, s)
        with pytest.raises(ValueError):
            PP.record_tables(s)


def test_writer_refuses_entries_the_rank_does_not_hold(tmp_path):
    rec = PP.VtuRecord.quads(np.array([[0, 0]]), 0.1, 0.1)
    rec.prs[2] = np.nan
    with pytest.raises(ValueError):
        PP.write_vtu_record(rec, str(tmp_path), "output", 0)


def test_triangle_record_against_the_ascii_writer(tmp_path):
    """The P2/P1 form: all vertices, a piece's cells — the arrays of `simplex.write_vtu` at its `%.16g`."""
    s = SX.build_space(G.read_msh(REF_MESH))
    rng = np.random.default_rng(2)
    u, p = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    for cells in (None, np.arange(len(s.cell_p))[::3]):
        rec = PP.VtuRecord.triangles(s.mesh.nodes, s.cell_p if cells is None else s.cell_p[cells])
        rec.vel3[:, 0], rec.vel3[:, 1], rec.prs[:] = u[0:2 * s.n_p:2], u[1:2 * s.n_p:2], p[:s.n_p]
        rec.write(str(tmp_path / "b.vtu"))
        SX.write_vtu(str(tmp_path / "a.vtu"), s, u, p, cells=cells)
        got, txt = VR.read(tmp_path / "b.vtu"), VR.read(tmp_path / "a.vtu")
        VR.check_layout(got, partitioning=False)
        assert got["point_data"] == txt["point_data"] and got["types"] == txt["types"]
        assert (got["n_points"], got["n_cells"]) == (txt["n_points"], txt["n_cells"]) == (s.n_p, len(s.cell_p if cells is None else cells))
        for name in txt["arrays"]:
            g = got["arrays"][name]
            if g.dtype == np.float64:                      # the ASCII file holds the values at its %.16g
                g = np.array(["%.16g" % v for v in g.reshape(-1)], float).reshape(g.shape)
            assert np.array_equal(g, txt["arrays"][name]), name
        assert np.all(got["arrays"]["types"] == 5) and got["arrays"]["velocity"][:, 2].tobytes() == np.zeros(s.n_p).tobytes()


# ---- the C++ writer ------------------------------------------------------------------------------------------------------
_CPP_MAIN = r"""
#include <cstdlib>
#include <vector>
#include "vtu_patches.hpp"
// argv: dir name counter n_digits rank nranks hx hy s file (int64 n, int32 ij[2n], double vel3[3 n (s+1)^2], double prs[n (s+1)^2])
int main(int, char **argv) {
  std::FILE *f = std::fopen(argv[10], "rb");
  const int s = std::atoi(argv[9]);
  int64_t n = 0;
  if (!f || std::fread(&n, 8, 1, f) != 1) return 1;
  const size_t np = (size_t)n * (s + 1) * (s + 1);
  std::vector<int32_t> ij(2 * n);
  if (std::fread(ij.data(), 4, 2 * n, f) != (size_t)(2 * n)) return 1;
  auto rec = vtu::quad_record(n, ij.data(), std::strtod(argv[7], nullptr), std::strtod(argv[8], nullptr), s, std::atoi(argv[5]));
  if ((size_t)rec->n_points() != np) return 2;
  if (std::fread(rec->vel3(), 8, 3 * np, f) != 3 * np || std::fread(rec->prs(), 8, np, f) != np) return 1;
  rec->write(argv[1], argv[2], vtu::counter_text(std::atoi(argv[3]), std::atoi(argv[4])), std::atoi(argv[5]), std::atoi(argv[6]));
  return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_writer(tmp_path_factory):
    d = tmp_path_factory.mktemp("cpp_record")
    src, exe = d / "main.cpp", d / "writer"
    src.write_text(_CPP_MAIN)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "navier_stokes_solver_amd", "csrc"), str(src),
                           "-o", str(exe)])
    return exe


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("nx,ny,lx", [(16, 10, 2.2), (4, 10, 0.44)])
def test_cpp_writer_is_the_python_writer_byte_for_byte(tmp_path, cpp_writer, nx, ny, lx, s):
    """csrc/vtu_patches.hpp (vtu::quad_record, the C++ drivers' record) in a stand-alone program: rank 1 of 2, and rank 0
    for the `.pvtu`."""
    hx, hy = lx / nx, PP.LY / ny
    for rank in (1, 0):
        _, ij = _strip(nx, ny, lx=lx, nranks=2, rank=rank)
        n = len(ij) * (s + 1) ** 2
        rng = np.random.default_rng(10 * s + rank)
        vel3, prs = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-14, 7, (n, 3)), rng.standard_normal(n)
        vel3[:, 2] = 0.0
        rec = PP.VtuRecord.quads(ij, hx, hy, s, rank)
        rec.vel3[:], rec.prs[:] = vel3, prs
        a, b = tmp_path / f"py{rank}", tmp_path / f"cpp{rank}"
        PP.write_vtu_record(rec, str(a), "output", 7, n_digits=3, rank=rank, nranks=2)
        blob = tmp_path / f"in{rank}.bin"
        blob.write_bytes(np.int64(len(ij)).tobytes() + ij.tobytes() + vel3.tobytes() + prs.tobytes())
        subprocess.check_call([str(cpp_writer), str(b), "output", "7", "3", str(rank), "2", repr(hx), repr(hy), str(s), str(blob)])
        files = sorted(os.listdir(a))
        assert files == sorted(os.listdir(b)) == ([f"output_007.{rank}.vtu"] + (["output_007.pvtu"] if rank == 0 else []))
        for name in files:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
        got = VR.read(b / f"output_007.{rank}.vtu")
        VR.check_layout(got)
        assert got["arrays"]["velocity"].tobytes() == vel3.tobytes() and np.all(got["arrays"]["partitioning"] == float(rank))


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_generator_tables_are_record_tables_bit_for_bit(s):
    L = P.lib()
    mesh = L.nsp_mesh_create(16, 10, 1, 0)
    try:
        wu, wp = PP.record_tables(s)
        assert wu.shape == ((s + 1) ** 2, 16) and wp.shape == ((s + 1) ** 2, 9)
        gu, gp = np.full_like(wu, np.nan), np.full_like(wp, np.nan)
        assert L.nsp_record_tables(mesh, s, gu.ctypes.data, gp.ctypes.data) == 0
        assert gu.tobytes() == wu.tobytes() and gp.tobytes() == wp.tobytes()
        assert L.nsp_record_tables(mesh, 5, gu.ctypes.data, gp.ctypes.data) != 0
        assert L.nsp_record_tables(mesh, 0, gu.ctypes.data, gp.ctypes.data) != 0
    finally:
        L.nsp_mesh_destroy(C.c_void_p(mesh))
    # each entry: the double product of two _lagrange values
    t = np.arange(s + 1) / s
    l3, l2 = PP._lagrange(PP._GLL, t)[0], PP._lagrange(PP._Q2, t)[0]
    for l in range(s + 1):
        for k in range(s + 1):
            pt = l * (s + 1) + k
            assert all(wu[pt, b * 4 + a] == l3[a, k] * l3[b, l] for b in range(4) for a in range(4))
            assert all(wp[pt, b * 3 + a] == l2[a, k] * l2[b, l] for b in range(3) for a in range(3))
    # rows at the vertex points: exact unit vectors at velocity nodes 0, 3, 12, 15 / pressure DoFs 0, 2, 6, 8
    for pt, un, pn in ((0, 0, 0), (s, 3, 2), (s * (s + 1), 12, 6), ((s + 1) ** 2 - 1, 15, 8)):
        assert np.array_equal(wu[pt], np.eye(16)[un]) and np.array_equal(wp[pt], np.eye(9)[pn])


@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 2)])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tables_reproduce_the_polynomials_of_the_spaces(nx, ny, s):
    """A bicubic velocity and a biquadratic pressure set at the nodes of every cell come back at all points of the record
    to 1e-13 of the field's size."""
    hx, hy = 0.7 / nx, 0.3 / ny
    wu, wp = PP.record_tables(s)
    vel = lambda x, y: (1.0 - 2.0 * x + 3.0 * x ** 3) * (0.5 + y - 4.0 * y ** 2 + 2.5 * y ** 3)      # noqa: E731
    prs = lambda x, y: (2.0 + x - 3.0 * x ** 2) * (1.0 - 0.5 * y + 6.0 * y ** 2)                      # noqa: E731
    t = np.arange(s + 1) / s
    for i in range(nx):
        for j in range(ny):
            for nodes, w, f in ((PP._GLL, wu, vel), (PP._Q2, wp, prs)):
                xn, yn = (i + nodes) * hx, (j + nodes) * hy
                at_nodes = np.array([f(xn[a], yn[b]) for b in range(len(nodes)) for a in range(len(nodes))])
                want = np.array([f((i + t[k]) * hx, (j + t[l]) * hy) for l in range(s + 1) for k in range(s + 1)])
                assert np.abs(w @ at_nodes - want).max() <= 1e-13 * np.abs(at_nodes).max()


# ---- the switches --------------------------------------------------------------------------------------------------------
def test_switches_parse_and_reject():
    assert cli.vtu_switches({}) == ("ascii", 1)
    assert cli.vtu_switches({"NSK_VTU_FORMAT": "ascii", "NSK_VTU_SUBDIVISIONS": "1"}) == ("ascii", 1)
    assert cli.vtu_switches({"NSK_VTU_FORMAT": "binary"}) == ("binary", 1)
    assert cli.vtu_switches({"NSK_VTU_FORMAT": "binary"}, read_mesh="mesh.msh") == ("binary", 1)
    assert cli.vtu_switches({"NSK_HOST_POSTPROCESS": "1"}) == ("ascii", 1)
    assert cli.vtu_switches({"NSK_VTU_FORMAT": "binary", "NSK_HOST_POSTPROCESS": "0"}) == ("binary", 1)
    for s in (2, 3, 4):
        assert cli.vtu_switches({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": str(s)}) == ("binary", s)
    rejected = [
        ({"NSK_VTU_FORMAT": "Binary"}, False), ({"NSK_VTU_FORMAT": ""}, False), ({"NSK_VTU_FORMAT": "base64"}, False),
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "0"}, False),
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "5"}, False),
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "2.0"}, False),
        ({"NSK_VTU_SUBDIVISIONS": ""}, False),
        ({"NSK_VTU_SUBDIVISIONS": "2"}, False),                                           # subdivided, ascii
        ({"NSK_VTU_FORMAT": "ascii", "NSK_VTU_SUBDIVISIONS": "3"}, False),
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "3"}, "mesh.msh"),           # subdivided, -M
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "3"}, True),
        ({"NSK_VTU_FORMAT": "binary", "NSK_VTU_SUBDIVISIONS": "3", "NSK_HOST_POSTPROCESS": "1"}, False),
        ({"NSK_VTU_FORMAT": "binary", "NSK_HOST_POSTPROCESS": "1"}, False),
    ]
    for env, read_mesh in rejected:
        with pytest.raises(ValueError, match=r"^NSK_VTU_\w+=\S* \S|^NSK_VTU_\w+=\S*: "):
            cli.vtu_switches(env, read_mesh)


def test_a_rejected_switch_ends_the_driver_before_anything_runs(monkeypatch, capsys):
    monkeypatch.setenv("NSK_VTU_SUBDIVISIONS", "2")
    monkeypatch.delenv("NSK_VTU_FORMAT", raising=False)
    assert cli.main(["StationaryNSSolver", "-m", "16,10"]) != 0
    out = capsys.readouterr()
    assert out.out == "" and out.err == "Error: NSK_VTU_SUBDIVISIONS=2 needs NSK_VTU_FORMAT=binary\n"


# ---- the reference of the s > 1 sums ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,lx,nranks,rank", [(16, 10, 2.2, 1, 0), (4, 10, 0.44, 2, 1)])
@pytest.mark.parametrize("s", [2, 3])
def test_reference_sums_against_plain_numpy(nx, ny, lx, nranks, rank, s):
    """The extended-precision statement within 17 u A_pt of a double evaluation: a product and at most 15 additions per
    elementary product of a 16-term sum in any order, one more unit for the second-order terms and the reference's own
    rounding."""
    one = P.generate(nx, ny, nu=0.1, lx=lx)
    pr = P.generate(nx, ny, nu=0.1, lx=lx, nranks=nranks, rank=rank)
    rng = np.random.default_rng(7)
    u, p = rng.standard_normal(one.info["n_u_global"]), rng.standard_normal(one.info["n_p_global"])
    ul, pl = local_state(pr, u, p)
    cells = np.nonzero(pr.cell_in_strip)[0]
    wu, wp = PP.record_tables(s)
    vel, prs, a_vel, a_prs = RR.record_sums(pr.cell_u_nodes, pr.cell_p_dofs, cells, wu, wp, ul, pl)
    assert vel.dtype == np.longdouble and vel.shape == (len(cells), (s + 1) ** 2, 2) and prs.shape == (len(cells), (s + 1) ** 2)
    un, pn = pr.cell_u_nodes[cells], pr.cell_p_dofs[cells]
    plain_v = np.stack([ul[2 * un] @ wu.T, ul[2 * un + 1] @ wu.T], axis=2)
    plain_p = pl[pn] @ wp.T
    assert (np.abs(plain_v - vel) <= 17 * U * a_vel).all() and (np.abs(plain_p - prs) <= 17 * U * a_prs).all()
    assert (a_vel >= np.abs(vel)).all() and (a_vel > 0).all() and (a_prs > 0).all()
    # at the vertex points: the entries of the state
    v = [0, s, s * (s + 1), (s + 1) ** 2 - 1]
    assert np.array_equal(vel[:, v, 0].astype(float), ul[2 * un[:, [0, 3, 12, 15]]])
    assert np.array_equal(prs[:, v].astype(float), pl[pn[:, [0, 2, 6, 8]]])
