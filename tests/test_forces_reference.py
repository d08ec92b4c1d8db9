"""Host side of the device report: the generator's obstacle faces and face tables, the extended-precision
statement of the force integral (tests/forces_reference.py) against the host yardstick `postprocess.lift_drag`, and the
patch-based VTU writers against `postprocess.write_vtu`, byte for byte.  No GPU."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from navier_stokes_solver_amd import postprocess as PP
from navier_stokes_solver_amd import problem as P
from tests import forces_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (nx, ny, lx, nranks): 4 x 10 on [0, 0.44]: the cells of the first 4 columns of a 20 x 10 mesh on the whole channel
MESHES = [(16, 10, 2.2, 1), (16, 10, 2.2, 2), (60, 20, 2.2, 1), (4, 10, 0.44, 1), (4, 10, 0.44, 2)]
SIDES = ((-1, 0), (1, 0), (0, -1), (0, 1))


def _kept(nx, ny, lx):
    """`Lattice.kept` of the nx columns on [0, lx]: the Lattice of the whole channel with the same cell width."""
    nx_full = int(round(nx * PP.LX / lx))
    assert abs(PP.LX / nx_full - lx / nx) < 1e-15
    return PP.Lattice(nx_full, ny).kept[:nx]


def _faces_of(kept, c0, c1):
    """Faces between a kept cell of columns [c0, c1) and a removed cell, sorted by (i, j, side)."""
    nx, ny = kept.shape
    out = []
    for i, j in zip(*np.nonzero(kept)):
        if c0 <= i < c1:
            for s, (di, dj) in enumerate(SIDES):
                ni, nj = i + di, j + dj
                if 0 <= ni < nx and 0 <= nj < ny and not kept[ni, nj]:
                    out.append((int(i), int(j), s))
    return out


@pytest.mark.parametrize("nx,ny,lx,nranks", MESHES)
def test_face_list_is_the_lattices(nx, ny, lx, nranks):
    kept = _kept(nx, ny, lx)
    cols = PP.cell_columns(nx, nranks)
    counts, sides = [], set()
    for r in range(nranks):
        pr = P.generate(nx, ny, nu=0.1, nranks=nranks, rank=r, lx=lx)
        assert pr.info["n_removed"] == int((~kept).sum())
        got = [(int(pr.cell_ij[c][0]), int(pr.cell_ij[c][1]), int(s)) for c, s in zip(pr.face_cell, pr.face_side)]
        assert got == _faces_of(kept, cols[r], cols[r + 1])
        assert pr.face_cell.dtype == np.int32 and pr.face_side.dtype == np.uint8
        # the strip's cells, in (i, j) order, are exactly the kept cells of its columns; the others are neighbours' cells
        own = pr.cell_ij[pr.cell_in_strip != 0]
        assert [tuple(c) for c in own] == [(i, j) for i, j in zip(*np.nonzero(kept)) if cols[r] <= i < cols[r + 1]]
        rest = pr.cell_ij[pr.cell_in_strip == 0]
        assert all(not cols[r] <= i < cols[r + 1] for i, _ in rest)
        counts.append(len(got))
        sides |= {s for _, _, s in got}
    if (nx, ny) == (16, 10):
        assert pr.info["n_removed"] == 2 and sum(counts) == 6
        assert sides == {0, 1, 2, 3}
        if nranks == 2:
            assert counts == [6, 0]                 # rank 1 owns no face
    if (nx, ny, nranks) == (4, 10, 2):
        # the cut falls at column 2, directly beside the hole at column 1
        assert cols == [0, 2, 4] and pr.info["n_removed"] == 2 and counts == [4, 2]
        assert not kept[1, 4] and not kept[1, 5]


@pytest.mark.parametrize("nx,ny,lx", [(16, 10, 2.2), (60, 20, 2.2), (4, 10, 0.44)])
def test_face_tables_are_the_lagrange_bases(nx, ny, lx):
    """Entry by entry against `postprocess._lagrange`, as `postprocess.lift_drag` tabulates a face, to 1e-14."""
    pr = P.generate(nx, ny, nu=0.1, lx=lx)
    tab = pr.face_tables
    assert tab.shape == (672,)
    hx, hy = lx / nx, PP.LY / ny
    gx, gw = np.polynomial.legendre.leggauss(4)
    gx, gw = 0.5 * (gx + 1.0), 0.5 * gw
    for s, (axis, fixed) in enumerate(((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0))):
        xs = np.full(4, fixed) if axis == 0 else gx
        ys = gx if axis == 0 else np.full(4, fixed)
        l3x, d3x = PP._lagrange(PP._GLL, xs)
        l3y, d3y = PP._lagrange(PP._GLL, ys)
        l2x, _ = PP._lagrange(PP._Q2, xs)
        l2y, _ = PP._lagrange(PP._Q2, ys)
        dx = np.array([d3x[a] * l3y[b] for b in range(4) for a in range(4)]) / hx
        dy = np.array([l3x[a] * d3y[b] for b in range(4) for a in range(4)]) / hy
        psi = np.array([l2x[a] * l2y[b] for b in range(3) for a in range(3)])
        for q in range(4):
            t = tab[(s * 4 + q) * 41:(s * 4 + q + 1) * 41]
            assert np.abs(t[:16] - dx[:, q]).max() <= 1e-14
            assert np.abs(t[16:32] - dy[:, q]).max() <= 1e-14
            assert np.abs(t[32:] - psi[:, q]).max() <= 1e-14
            assert abs(tab[656 + s * 4 + q] - gw[q] * (hy if axis == 0 else hx)) <= 1e-14


def _random_state(pr, seed):
    rng = np.random.default_rng(seed)
    i = pr.info
    return rng.standard_normal(i["n_u_global"]), rng.standard_normal(i["n_p_global"])


@pytest.mark.parametrize("nx,ny,nranks", [(16, 10, 1), (16, 10, 2), (60, 20, 1), (60, 20, 3)])
@pytest.mark.parametrize("nu", [0.37, 0.0])
def test_reference_formula_is_lift_drag(nx, ny, nranks, nu):
    """The extended-precision statement from the hand-off equals the host yardstick, rank share by rank share, within
    1e-12 A on random fields."""
    u, p = _random_state(P.generate(nx, ny, nu=0.1), 5)
    for r in range(nranks):
        pr = P.generate(nx, ny, nu=0.1, nranks=nranks, rank=r)
        ul, pl = R.local_state(pr, u, p)
        (drag, lift), (a_d, a_l) = R.q3_forces(pr.cell_u_nodes, pr.cell_p_dofs, pr.face_cell, pr.face_side, pr.face_tables,
                                               ul, pl, nu)
        d0, l0 = PP.lift_drag(nx, ny, u, p, nu, rank=r, nranks=nranks)
        assert a_d >= abs(drag) and a_l >= abs(lift)
        assert abs(float(drag) - d0) <= 1e-12 * float(a_d) and abs(float(lift) - l0) <= 1e-12 * float(a_l)
        if len(pr.face_cell):
            assert a_d > 0 and a_l > 0
        else:
            assert drag == 0 and lift == 0 and a_d == 0


def _patches(L, ij, u, p):
    """What `nsk_state_get_patches` returns for the cells ij, from global vectors."""
    corners = ((0, 0), (1, 0), (0, 1), (1, 1))
    un = np.array([[L.uid[3 * (i + a), 3 * (j + b)] for a, b in corners] for i, j in ij]).reshape(-1, 4)
    pn = np.array([[L.pid[2 * (i + a), 2 * (j + b)] for a, b in corners] for i, j in ij]).reshape(-1, 4)
    return np.stack([u[2 * un], u[2 * un + 1]], axis=2), p[pn]


def _awkward_state(L):
    rng = np.random.default_rng(11)
    u = rng.standard_normal(L.n_u) * 10.0 ** rng.integers(-14, 7, L.n_u)      # every branch of %.12g: fixed, exponent
    p = rng.standard_normal(L.n_p) * 10.0 ** rng.integers(-5, 18, L.n_p)
    u[:6] = [0.0, -0.0, 1e-300, 123456789012.5, 0.1, -1.0]
    return u, p


@pytest.mark.parametrize("nranks", [1, 3])
@pytest.mark.parametrize("name,counter,n_digits", [("output-stokes", 0, None), ("output", 7, 3), ("output", 1234, 3)])
def test_patch_writer_is_write_vtu_byte_for_byte(tmp_path, nranks, name, counter, n_digits):
    nx, ny = 16, 10
    L = PP.Lattice(nx, ny)
    u, p = _awkward_state(L)
    a, b = tmp_path / "a", tmp_path / "b"
    for r in range(nranks):
        pr = P.generate(nx, ny, nu=0.1, nranks=nranks, rank=r)
        ij = pr.cell_ij[pr.cell_in_strip != 0]
        vel, prs = _patches(L, ij, u, p)
        f0 = PP.write_vtu(str(a), name, counter, nx, ny, u, p, n_digits=n_digits, rank=r, nranks=nranks)
        f1 = PP.write_vtu_patches(str(b), name, counter, ij, PP.LX / nx, PP.LY / ny, vel, prs, n_digits=n_digits, rank=r,
                                  nranks=nranks)
        assert os.path.basename(f0) == os.path.basename(f1)
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and len(files) == nranks + 1
    assert filecmp.cmpfiles(a, b, files, shallow=False) == (files, [], [])


def test_patch_writer_refuses_entries_the_rank_does_not_hold(tmp_path):
    ij = np.array([[0, 0]])
    vel, prs = np.zeros((1, 4, 2)), np.zeros((1, 4))
    vel[0, 2, 1] = np.nan
    with pytest.raises(ValueError):
        PP.write_vtu_patches(str(tmp_path), "output", 0, ij, 0.1, 0.1, vel, prs)


_CPP_MAIN = r"""
#include <cstdlib>
#include <vector>
#include "vtu_patches.hpp"
// argv: dir name counter n_digits rank nranks hx hy file (int64 n, int32 ij[2n], double vel[8n], double prs[4n])
int main(int, char **argv) {
  std::FILE *f = std::fopen(argv[9], "rb");
  int64_t n = 0;
  if (!f || std::fread(&n, 8, 1, f) != 1) return 1;
  std::vector<int32_t> ij(2 * n);
  std::vector<double> vel(8 * n), prs(4 * n);
  if (std::fread(ij.data(), 4, 2 * n, f) != (size_t)(2 * n) || std::fread(vel.data(), 8, 8 * n, f) != (size_t)(8 * n) ||
      std::fread(prs.data(), 8, 4 * n, f) != (size_t)(4 * n)) return 1;
  vtu::write_patches(argv[1], argv[2], vtu::counter_text(std::atoi(argv[3]), std::atoi(argv[4])), n, ij.data(),
                     std::strtod(argv[7], nullptr), std::strtod(argv[8], nullptr), vel.data(), prs.data(), std::atoi(argv[5]),
                     std::atoi(argv[6]));
  return 0;
}
"""


def test_cpp_writer_is_the_python_writer_byte_for_byte(tmp_path):
    """csrc/vtu_patches.hpp (the C++ drivers' record) in a stand-alone program against `write_vtu_patches`."""
    src, exe = tmp_path / "main.cpp", tmp_path / "writer"
    src.write_text(_CPP_MAIN)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "navier_stokes_solver_amd", "csrc"), str(src),
                           "-o", str(exe)])
    nx, ny = 16, 10
    L = PP.Lattice(nx, ny)
    u, p = _awkward_state(L)
    pr = P.generate(nx, ny, nu=0.1)
    ij = np.ascontiguousarray(pr.cell_ij, np.int32)
    vel, prs = _patches(L, ij, u, p)
    blob = tmp_path / "in.bin"
    blob.write_bytes(np.int64(len(ij)).tobytes() + ij.tobytes() + np.ascontiguousarray(vel).tobytes() +
                     np.ascontiguousarray(prs).tobytes())
    for rank, nranks, name, counter, nd in ((0, 1, "output-stokes", 0, 0), (0, 2, "output", 7, 3), (1, 2, "output", 7, 3)):
        a, b = tmp_path / f"py{rank}{nranks}", tmp_path / f"cpp{rank}{nranks}"
        PP.write_vtu_patches(str(a), name, counter, ij, PP.LX / nx, PP.LY / ny, vel, prs, n_digits=nd or None, rank=rank,
                             nranks=nranks)
        subprocess.check_call([str(exe), str(b), name, str(counter), str(nd), str(rank), str(nranks), repr(PP.LX / nx),
                               repr(PP.LY / ny), str(blob)])
        files = sorted(os.listdir(a))
        assert files == sorted(os.listdir(b)) and len(files) == (2 if rank == 0 else 1)
        assert filecmp.cmpfiles(a, b, files, shallow=False) == (files, [], [])
