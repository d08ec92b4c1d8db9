"""Consumers of the solution, host side: lift / drag over the obstacle boundary and VTU output.
`lift_drag` and `write_vtu` work on downloaded global vectors and are the yardsticks of the device path (`nsk_forces`,
`nsk_state_get_patches` + `write_vtu_patches`), which the drivers use.

Reference: `NSSolverStationary::compute_lift_drag()`, `compute_lift_coeff()`, `compute_drag_coeff()`, `output()`
(lab_new/src/NSSolverStationary.cpp:765-800, 802-897, 905-933) and the NSSolver twins (NSSolver.cpp:761-797,
839-975).  These read the solution once per Newton pass / time step; they are not on the accelerated path and
work on the vectors the drivers download with `nsk_state_get`.

Several ranks (x-strips of whole cell columns, the generator's partition): every rank integrates / writes ITS cells —
`lift_drag(..., rank, nranks)` returns the rank's share, which `sum_over_ranks` adds up as the reference's
`Utilities::MPI::sum` does (.cpp:895-896; NSSolver.cpp:933-934); `write_vtu(..., rank, nranks)` writes the rank's
piece and, on rank 0, the `.pvtu` record naming all pieces (`write_vtu_with_pvtu_record`, .cpp:793-796).  A rank only
touches entries of its owned and ghost DoFs: `global_view` scatters them into global numbering (NaN elsewhere).

The generated mesh is the nx x ny lattice over [0, 2.2] x [0, 0.41] without the cells whose centre is closer than
0.05 to (0.2, 0.205) (`NSSolverStationary.cpp:13-63`); boundary id 10 (the obstacle) is every face between a kept
and a removed cell.  DoF numbering: lattice nodes x-major, two velocity components per Q3 node.
"""
from __future__ import annotations

import os

import numpy as np

LX, LY, HX, HY, R = 2.2, 0.41, 0.2, 0.205, 0.05
_GLL = np.array([0.0, 0.5 * (1 - 1 / np.sqrt(5)), 0.5 * (1 + 1 / np.sqrt(5)), 1.0])
_Q2 = np.array([0.0, 0.5, 1.0])


def _lagrange(nodes, x):
    """Values and derivatives of the Lagrange basis on `nodes` at the points x: arrays [basis, point]."""
    x = np.atleast_1d(np.asarray(x, float))
    n = len(nodes)
    val, der = np.ones((n, x.size)), np.zeros((n, x.size))
    for a in range(n):
        for b in range(n):
            if b != a:
                val[a] *= (x - nodes[b]) / (nodes[a] - nodes[b])
        for b in range(n):
            if b == a:
                continue
            t = np.full(x.size, 1.0 / (nodes[a] - nodes[b]))
            for c in range(n):
                if c not in (a, b):
                    t *= (x - nodes[c]) / (nodes[a] - nodes[c])
            der[a] += t
    return val, der


class Lattice:
    """Kept cells and the node numbering of the generated mesh."""

    def __init__(self, nx, ny):
        self.nx, self.ny = nx, ny
        self.hx, self.hy = LX / nx, LY / ny
        cx = (np.arange(nx) + 0.5) * self.hx
        cy = (np.arange(ny) + 0.5) * self.hy
        self.kept = np.hypot(cx[:, None] - HX, cy[None, :] - HY) >= R
        self.uid = self._number(3)
        self.pid = self._number(2)
        self.n_u = 2 * (int(self.uid.max()) + 1)
        self.n_p = int(self.pid.max()) + 1

    def _number(self, step):
        used = np.zeros((step * self.nx + 1, step * self.ny + 1), bool)
        for i, j in zip(*np.nonzero(self.kept)):
            used[step * i:step * i + step + 1, step * j:step * j + step + 1] = True
        ids = -np.ones(used.shape, np.int64)
        ids[used] = np.arange(int(used.sum()))      # row-major over (ix, iy) = x-major
        return ids

    def is_kept(self, i, j):
        return 0 <= i < self.nx and 0 <= j < self.ny and bool(self.kept[i, j])

    def cell_nodes(self, i, j):
        un = np.array([self.uid[3 * i + a, 3 * j + b] for b in range(4) for a in range(4)])
        pn = np.array([self.pid[2 * i + a, 2 * j + b] for b in range(3) for a in range(3)])
        return un, pn


def cell_columns(nx, nranks):
    """First cell column of every rank's x-strip (+ end): the generator's rule (csrc/problem_gen.cpp)."""
    return [r * nx // nranks for r in range(nranks + 1)]


def global_view(n_global, begin, owned, ghost_ids, ghost):
    """A rank's owned + ghost entries in GLOBAL numbering, NaN where the rank holds nothing (velocity: pass DoF ids)."""
    g = np.full(n_global, np.nan)
    g[begin:begin + len(owned)] = owned
    g[np.asarray(ghost_ids, np.int64)] = ghost
    return g


def sum_over_ranks(values):
    """`Utilities::MPI::sum` over the ranks of the running torch.distributed job (identity on one rank)."""
    try:
        import torch
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor(list(values), dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return tuple(float(v) for v in t)
    except ImportError:
        pass
    return tuple(float(v) for v in values)


def lift_drag(nx, ny, u, p, nu, rank=0, nranks=1):
    """(drag_force, lift_force): -sum over the obstacle faces of (nu (grad u + grad u^T) - p I) n JxW with the
    fluid cell's outward normal, 4 Gauss points per face (NSSolverStationary.cpp:844-892).  With several ranks: the
    share of the cells of this rank's strip (add the shares with `sum_over_ranks`)."""
    L = Lattice(nx, ny)
    u, p = np.asarray(u, float), np.asarray(p, float)
    if u.shape != (L.n_u,) or p.shape != (L.n_p,):
        raise ValueError("solution vectors do not match the mesh")
    c0, c1 = cell_columns(nx, nranks)[rank:rank + 2]
    gx, gw = np.polynomial.legendre.leggauss(4)
    gx, gw = 0.5 * (gx + 1.0), 0.5 * gw
    drag = lift = 0.0
    faces = (((-1, 0), 0, 0.0), ((1, 0), 0, 1.0), ((0, -1), 1, 0.0), ((0, 1), 1, 1.0))   # neighbour, fixed axis, coordinate
    for i, j in zip(*np.nonzero(L.kept)):
        if not c0 <= i < c1:
            continue                          # another rank's cell
        for (di, dj), axis, fixed in faces:
            ni, nj = i + di, j + dj
            if not (0 <= ni < nx and 0 <= nj < ny) or L.kept[ni, nj]:
                continue                      # outer boundary (ids 6, 7, 8) or interior face
            un, pn = L.cell_nodes(i, j)
            xs = np.full(4, fixed) if axis == 0 else gx
            ys = gx if axis == 0 else np.full(4, fixed)
            l3x, d3x = _lagrange(_GLL, xs)
            l3y, d3y = _lagrange(_GLL, ys)
            l2x, _ = _lagrange(_Q2, xs)
            l2y, _ = _lagrange(_Q2, ys)
            phi_dx = np.array([d3x[a] * l3y[b] for b in range(4) for a in range(4)]) / L.hx      # [n, q]
            phi_dy = np.array([l3x[a] * d3y[b] for b in range(4) for a in range(4)]) / L.hy
            psi = np.array([l2x[a] * l2y[b] for b in range(3) for a in range(3)])
            ux, uy = u[2 * un], u[2 * un + 1]
            g = np.array([[ux @ phi_dx, ux @ phi_dy], [uy @ phi_dx, uy @ phi_dy]])                # [k, l, q]
            pq = p[pn] @ psi
            jxw = gw * (L.hy if axis == 0 else L.hx)
            n = np.array([di, dj], float)     # outward normal of the fluid cell
            for q in range(4):
                s = nu * (g[:, :, q] + g[:, :, q].T) - pq[q] * np.eye(2)
                f = -(s @ n) * jxw[q]
                drag += f[0]
                lift += f[1]
    if not (np.isfinite(drag) and np.isfinite(lift)):
        raise ValueError("lift/drag touched an entry this rank does not hold (owned + ghost DoFs)")
    return float(drag), float(lift)


def coefficients(drag_force, lift_force, inlet_u):
    """2 F / (U_avg^2 D) with U_avg = 2 U(0, H/2) / 3 and D = 0.1 (NSSolverStationary.cpp:899-919)."""
    u_avg = 2.0 * inlet_u / 3.0
    return 2.0 * drag_force / (u_avg * u_avg * 0.1), 2.0 * lift_force / (u_avg * u_avg * 0.1)


def write_vtu(directory, name, counter, nx, ny, u, p, n_digits=None, rank=0, nranks=1):
    """`DataOut::write_vtu_with_pvtu_record`: this rank's piece `<name>_<counter>.<rank>.vtu` (its strip of cells)
    and, on rank 0, the record `<name>_<counter>.pvtu` naming the pieces of all ranks.  As deal.II's default
    `build_patches()` does, every cell is one patch with its own four vertices; point data `velocity` (3 components,
    z = 0), `pressure`, `partitioning` (NSSolverStationary.cpp:769-796).  ASCII XML."""
    L = Lattice(nx, ny)
    c0, c1 = cell_columns(nx, nranks)[rank:rank + 2]
    cells = np.array([c for c in np.argwhere(L.kept) if c0 <= c[0] < c1]).reshape(-1, 2)
    pts, vel, prs = [], [], []
    for i, j in cells:
        for (a, b) in ((0, 0), (1, 0), (0, 1), (1, 1)):          # deal.II vertex order of a patch
            ix, iy = i + a, j + b
            pts.append((ix * L.hx, iy * L.hy, 0.0))
            node = L.uid[3 * ix, 3 * iy]
            vel.append((u[2 * node], u[2 * node + 1], 0.0))
            prs.append(p[L.pid[2 * ix, 2 * iy]])
    if not (np.isfinite(np.asarray(vel)).all() and np.isfinite(np.asarray(prs)).all()):
        raise ValueError("VTU output touched an entry this rank does not hold (owned + ghost DoFs)")
    n_cells, n_pts = len(cells), len(pts)
    cnt = str(counter) if n_digits is None else str(counter).zfill(n_digits)
    piece = f"{name}_{cnt}.{rank}.vtu"
    fmt = lambda rows: "\n".join(" ".join(f"{v:.12g}" for v in np.atleast_1d(r)) for r in rows)   # noqa: E731
    conn = "\n".join(f"{4 * c} {4 * c + 1} {4 * c + 3} {4 * c + 2}" for c in range(n_cells))       # VTK_QUAD ordering
    xml = f"""<?xml version="1.0" ?>
<VTKFile type="UnstructuredGrid" version="0.1" byte_order="LittleEndian">
<UnstructuredGrid>
<Piece NumberOfPoints="{n_pts}" NumberOfCells="{n_cells}">
<Points>
<DataArray type="Float64" NumberOfComponents="3" format="ascii">
{fmt(pts)}
</DataArray>
</Points>
<Cells>
<DataArray type="Int32" Name="connectivity" format="ascii">
{conn}
</DataArray>
<DataArray type="Int32" Name="offsets" format="ascii">
{" ".join(str(4 * (c + 1)) for c in range(n_cells))}
</DataArray>
<DataArray type="UInt8" Name="types" format="ascii">
{" ".join("9" for _ in range(n_cells))}
</DataArray>
</Cells>
<PointData Scalars="scalars">
<DataArray type="Float64" Name="velocity" NumberOfComponents="3" format="ascii">
{fmt(vel)}
</DataArray>
<DataArray type="Float64" Name="pressure" format="ascii">
{fmt(prs)}
</DataArray>
<DataArray type="Float64" Name="partitioning" format="ascii">
{" ".join(str(float(rank)) for _ in range(n_pts))}
</DataArray>
</PointData>
</Piece>
</UnstructuredGrid>
</VTKFile>
"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, piece), "w") as f:
        f.write(xml)
    if rank != 0:
        return os.path.join(directory, piece)
    pieces = "\n".join(f'<Piece Source="{name}_{cnt}.{r}.vtu"/>' for r in range(nranks))
    pvtu = f"""<?xml version="1.0"?>
<VTKFile type="PUnstructuredGrid" version="0.1" byte_order="LittleEndian">
<PUnstructuredGrid GhostLevel="0">
<PPointData Scalars="scalars">
<PDataArray type="Float64" Name="velocity" NumberOfComponents="3" format="ascii"/>
<PDataArray type="Float64" Name="pressure" format="ascii"/>
<PDataArray type="Float64" Name="partitioning" format="ascii"/>
</PPointData>
<PPoints>
<PDataArray type="Float64" NumberOfComponents="3"/>
</PPoints>
{pieces}
</PUnstructuredGrid>
</VTKFile>
"""
    with open(os.path.join(directory, f"{name}_{cnt}.pvtu"), "w") as f:
        f.write(pvtu)
    return os.path.join(directory, piece)


def _join_rows(a):
    """`write_vtu`'s number formatting (`.12g`) of a 2-D array: one row per line, entries separated by blanks."""
    t = np.char.mod("%.12g", np.asarray(a, float))
    out = t[:, 0]
    for k in range(1, t.shape[1]):
        out = np.char.add(np.char.add(out, " "), t[:, k])
    return "\n".join(out.tolist())


def _write_pvtu(directory, name, cnt, nranks, fields=()):
    """The record `<name>_<cnt>.pvtu` naming the pieces of all ranks, as `write_vtu` writes it; `fields`: the derived arrays
    of the pieces, listed after `pressure`."""
    pieces = "\n".join(f'<Piece Source="{name}_{cnt}.{r}.vtu"/>' for r in range(nranks))
    extra = "".join(f'<PDataArray type="Float64" Name="{f}" format="ascii"/>\n' for f in fields)
    pvtu = f"""<?xml version="1.0"?>
<VTKFile type="PUnstructuredGrid" version="0.1" byte_order="LittleEndian">
<PUnstructuredGrid GhostLevel="0">
<PPointData Scalars="scalars">
<PDataArray type="Float64" Name="velocity" NumberOfComponents="3" format="ascii"/>
<PDataArray type="Float64" Name="pressure" format="ascii"/>
{extra}<PDataArray type="Float64" Name="partitioning" format="ascii"/>
</PPointData>
<PPoints>
<PDataArray type="Float64" NumberOfComponents="3"/>
</PPoints>
{pieces}
</PUnstructuredGrid>
</VTKFile>
"""
    with open(os.path.join(directory, f"{name}_{cnt}.pvtu"), "w") as f:
        f.write(pvtu)


def write_vtu_patches(directory, name, counter, ij, hx, hy, vel, prs, n_digits=None, rank=0, nranks=1):
    """The files `write_vtu` writes, byte for byte, from per-cell patches instead of global vectors: `ij` [n, 2] the lattice
    positions of this rank's cells in (i, j) order, `vel` [n, 4, 2] and `prs` [n, 4] the state at their vertices (0,0), (1,0),
    (0,1), (1,1) (`LinearSolver.state_patches`).  No loop over the cells in Python."""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    vel = np.asarray(vel, float).reshape(-1, 4, 2)
    prs = np.asarray(prs, float).reshape(-1, 4)
    n_cells = len(ij)
    if vel.shape[0] != n_cells or prs.shape[0] != n_cells:
        raise ValueError("patches do not match the cell list")
    if not (np.isfinite(vel).all() and np.isfinite(prs).all()):
        raise ValueError("VTU output touched an entry this rank does not hold (owned + ghost DoFs)")
    n_pts = 4 * n_cells
    da, db = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1])          # deal.II vertex order of a patch
    zero = np.zeros((n_pts, 1))
    pts = np.concatenate([((ij[:, :1] + da).reshape(-1, 1)) * hx, ((ij[:, 1:] + db).reshape(-1, 1)) * hy, zero], axis=1)
    cnt = str(counter) if n_digits is None else str(counter).zfill(n_digits)
    piece = f"{name}_{cnt}.{rank}.vtu"
    c4 = 4 * np.arange(n_cells).reshape(-1, 1)
    ints = lambda a: np.char.mod("%d", a)                            # noqa: E731
    conn = ints(c4 + np.array([0, 1, 3, 2]))                         # VTK_QUAD ordering
    conn = "\n".join(np.char.add(np.char.add(np.char.add(conn[:, 0], " "), np.char.add(conn[:, 1], " ")),
                                 np.char.add(np.char.add(conn[:, 2], " "), conn[:, 3])).tolist()) if n_cells else ""
    xml = f"""<?xml version="1.0" ?>
<VTKFile type="UnstructuredGrid" version="0.1" byte_order="LittleEndian">
<UnstructuredGrid>
<Piece NumberOfPoints="{n_pts}" NumberOfCells="{n_cells}">
<Points>
<DataArray type="Float64" NumberOfComponents="3" format="ascii">
{_join_rows(pts) if n_cells else ""}
</DataArray>
</Points>
<Cells>
<DataArray type="Int32" Name="connectivity" format="ascii">
{conn}
</DataArray>
<DataArray type="Int32" Name="offsets" format="ascii">
{" ".join(ints(4 * np.arange(1, n_cells + 1)).tolist())}
</DataArray>
<DataArray type="UInt8" Name="types" format="ascii">
{" ".join(["9"] * n_cells)}
</DataArray>
</Cells>
<PointData Scalars="scalars">
<DataArray type="Float64" Name="velocity" NumberOfComponents="3" format="ascii">
{_join_rows(np.concatenate([vel.reshape(-1, 2), zero], axis=1)) if n_cells else ""}
</DataArray>
<DataArray type="Float64" Name="pressure" format="ascii">
{_join_rows(prs.reshape(-1, 1)) if n_cells else ""}
</DataArray>
<DataArray type="Float64" Name="partitioning" format="ascii">
{" ".join([str(float(rank))] * n_pts)}
</DataArray>
</PointData>
</Piece>
</UnstructuredGrid>
</VTKFile>
"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, piece), "w") as f:
        f.write(xml)
    if rank != 0:
        return os.path.join(directory, piece)
    _write_pvtu(directory, name, cnt, nranks)
    return os.path.join(directory, piece)


# ---- the record as VTK XML with raw appended data ----
def record_tables(s):
    """(w_u [(s+1)^2, 16], w_p [(s+1)^2, 9]) of `nsk_record_set_cells`: the Q3 (GLL nodes) and Q2 bases of a cell at its
    (s+1)^2 lattice points, pt = l (s+1) + k at (k / s, l / s); w_u[pt, b*4 + a] = L_a(t_k) L_b(t_l), each entry the
    double product of two `_lagrange` values (csrc/problem_gen.cpp::nsp_record_tables gives the same bits)."""
    if s not in (1, 2, 3, 4):
        raise ValueError("subdivisions must be 1, 2, 3 or 4")
    t = np.arange(s + 1) / s
    out = []
    for nodes in (_GLL, _Q2):
        a = _lagrange(nodes, t)[0].T                                   # [point, basis]
        n = len(nodes)
        out.append((a[None, :, None, :] * a[:, None, :, None]).reshape((s + 1) ** 2, n * n))    # [l, k, b, a]
    return out[0], out[1]


FIELDS = ("vorticity", "divergence")        # the derived arrays of the record, in file order; bit k of the library's mask


def record_gradient_tables(s, hx, hy):
    """(d_x, d_y) [(s+1)^2, 16] of `nsk_record_set_gradient`, laid out like `record_tables`' w_u:
    d_x[pt, b*4 + a] = L'_a(t_k) L_b(t_l) / hx and d_y[pt, b*4 + a] = L_a(t_k) L'_b(t_l) / hy on the GLL nodes, each entry the
    double product of two `_lagrange` values followed by one division (csrc/problem_gen.cpp::nsp_record_gradient_tables gives
    the same bits)."""
    if s not in (1, 2, 3, 4):
        raise ValueError("subdivisions must be 1, 2, 3 or 4")
    if not (hx > 0.0 and hy > 0.0):
        raise ValueError("cell sizes must be positive")
    val, der = _lagrange(_GLL, np.arange(s + 1) / s)
    v, d = val.T, der.T                                                # [point, basis]
    dx = (d[None, :, None, :] * v[:, None, :, None]).reshape((s + 1) ** 2, 16) / float(hx)       # [l, k, b, a]
    dy = (v[None, :, None, :] * d[:, None, :, None]).reshape((s + 1) ** 2, 16) / float(hy)
    return dx, dy


def field_mask(fields):
    """The mask of `nsk_state_get_record_fields` for a tuple of names out of `FIELDS`."""
    m = 0
    for f in fields:
        if f not in FIELDS:
            raise ValueError(f"unknown record field {f!r}")
        m |= 1 << FIELDS.index(f)
    return m


class VtuRecord:
    """The image of one `.vtu` piece in VTK's XML format with raw appended data, built once per run and rank: the XML
    header, then after `<AppendedData encoding="raw">` and `_` the blocks — a UInt64 byte count and that many bytes each —
    points, `velocity`, `pressure`, [`vorticity`,] [`divergence`,] [`partitioning`,] `connectivity`, `offsets`, `types`.  The
    header is padded with blanks so that the first block starts at a multiple of 8 in the file.  Everything but `velocity`,
    `pressure` and the derived arrays is filled in here; `vel3` [n, 3] and `prs` [n] are views of the image at those two
    blocks — a report fills them (`LinearSolver.state_record(vel3=..., prs=...)`) and writes the image with one write.
    `fields`: names out of `FIELDS`; each becomes one Float64 array of one component after `pressure`, in the
    order of `FIELDS`, and `field[name]` [n] is the view a report fills (`LinearSolver.record_fields`).  With no fields the
    image is the one without them, byte for byte."""

    def __init__(self, points, connectivity, offsets, types, partitioning=None, declaration='<?xml version="1.0" ?>',
                 point_data='Scalars="scalars"', fields=()):
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        conn = np.ascontiguousarray(connectivity, np.int32).reshape(-1)
        offs = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        typ = np.ascontiguousarray(types, np.uint8).reshape(-1)
        n, m = len(pts), len(offs)
        if len(typ) != m:
            raise ValueError("offsets and types do not match")
        field_mask(fields)
        self.fields = tuple(f for f in FIELDS if f in fields)
        blocks = [("points", pts), ("velocity", 24 * n), ("pressure", 8 * n)] + [(f, 8 * n) for f in self.fields]
        if partitioning is not None:
            blocks.append(("partitioning", np.full(n, float(partitioning))))
        blocks += [("connectivity", conn), ("offsets", offs), ("types", typ)]
        at, pos = {}, 0
        for key, b in blocks:
            at[key] = pos
            pos += 8 + (b if isinstance(b, int) else b.nbytes)
        arr = lambda typ_, key, extra="": (f'<DataArray type="{typ_}"' + (f' Name="{key}"' if key != "points" else "") +   # noqa: E731
                                           f'{extra} format="appended" offset="{at[key]}"/>\n')
        head = (f'{declaration}\n<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
                f'<UnstructuredGrid>\n<Piece NumberOfPoints="{n}" NumberOfCells="{m}">\n<Points>\n'
                + arr("Float64", "points", ' NumberOfComponents="3"') + "</Points>\n<Cells>\n" + arr("Int32", "connectivity")
                + arr("Int32", "offsets") + arr("UInt8", "types") + f"</Cells>\n<PointData {point_data}>\n"
                + arr("Float64", "velocity", ' NumberOfComponents="3"') + arr("Float64", "pressure")
                + "".join(arr("Float64", f) for f in self.fields)
                + (arr("Float64", "partitioning") if partitioning is not None else "")
                + "</PointData>\n</Piece>\n</UnstructuredGrid>\n")
        opening = '<AppendedData encoding="raw">\n_'
        head += " " * (-(len(head) + len(opening)) % 8) + opening
        closing = b"\n</AppendedData>\n</VTKFile>\n"
        start = len(head)
        self.image = np.zeros(start + pos + len(closing), np.uint8)
        self.image[:start] = np.frombuffer(head.encode("ascii"), np.uint8)
        self.image[start + pos:] = np.frombuffer(closing, np.uint8)
        for key, b in blocks:
            o = start + at[key]
            nbytes = b if isinstance(b, int) else b.nbytes
            self.image[o:o + 8] = np.frombuffer(np.uint64(nbytes).tobytes(), np.uint8)
            if not isinstance(b, int):
                self.image[o + 8:o + 8 + nbytes] = b.reshape(-1).view(np.uint8)
        self.n_points, self.n_cells = n, m
        self.vel3 = self.image[start + at["velocity"] + 8:start + at["velocity"] + 8 + 24 * n].view(np.float64).reshape(n, 3)
        self.prs = self.image[start + at["pressure"] + 8:start + at["pressure"] + 8 + 8 * n].view(np.float64)
        self.field = {f: self.image[start + at[f] + 8:start + at[f] + 8 + 8 * n].view(np.float64) for f in self.fields}

    @classmethod
    def quads(cls, ij, hx, hy, subdivisions=1, rank=0, fields=()):
        """The piece of the generated mesh's cells `ij` [n, 2] in file order: per cell (s+1)^2 points ((i + k/s) hx,
        (j + l/s) hy, 0), pt = l (s+1) + k, and s^2 VTK_QUADs base + l (s+1) + k, +1, +(s+1)+1, +(s+1) — for s = 1 the
        points and the `0 1 3 2` of `write_vtu_patches`."""
        s = int(subdivisions)
        if s not in (1, 2, 3, 4):
            raise ValueError("subdivisions must be 1, 2, 3 or 4")
        ij = np.asarray(ij, np.int64).reshape(-1, 2)
        n_cells, ppc = len(ij), (s + 1) ** 2
        t = np.arange(s + 1) / s
        pts = np.zeros((n_cells, s + 1, s + 1, 3))                                  # [cell, l, k]
        pts[..., 0] = ((ij[:, 0, None] + t[None, :]) * hx)[:, None, :]
        pts[..., 1] = ((ij[:, 1, None] + t[None, :]) * hy)[:, :, None]
        l, k = np.divmod(np.arange(s * s), s)
        first = (l * (s + 1) + k)[:, None] + np.array([0, 1, s + 2, s + 1])        # VTK_QUAD ordering
        conn = ppc * np.arange(n_cells)[:, None, None] + first[None]
        n_quads = n_cells * s * s
        return cls(pts.reshape(-1, 3), conn, 4 * np.arange(1, n_quads + 1), np.full(n_quads, 9), partitioning=rank,
                   fields=fields)

    @classmethod
    def triangles(cls, nodes, cells, fields=()):
        """The piece `simplex.write_vtu` writes: all vertices `nodes` [n, 2], the piece's linear triangles `cells` [m, 3]."""
        nodes = np.asarray(nodes, float).reshape(-1, 2)
        cells = np.asarray(cells).reshape(-1, 3)
        pts = np.concatenate([nodes, np.zeros((len(nodes), 1))], axis=1)
        return cls(pts, cells, 3 * np.arange(1, len(cells) + 1), np.full(len(cells), 5), declaration='<?xml version="1.0"?>',
                   point_data='Vectors="velocity" Scalars="pressure"', fields=fields)

    def write(self, path):
        """The image as it stands, with one write."""
        if not (np.isfinite(self.vel3).all() and np.isfinite(self.prs).all() and all(np.isfinite(a).all() for a in self.field.values())):
            raise ValueError("VTU output touched an entry this rank does not hold (owned + ghost DoFs)")
        with open(path, "wb") as f:
            f.write(self.image)
        return path


def write_vtu_record(record, directory, name, counter, n_digits=None, rank=0, nranks=1):
    """The files of `write_vtu_patches` with the piece as `record`'s image (a `VtuRecord` whose `vel3` / `prs` hold the
    values): `<name>_<counter>.<rank>.vtu` and, on rank 0, the same `.pvtu`, byte for byte."""
    cnt = str(counter) if n_digits is None else str(counter).zfill(n_digits)
    os.makedirs(directory, exist_ok=True)
    piece = record.write(os.path.join(directory, f"{name}_{cnt}.{rank}.vtu"))
    if rank == 0:
        _write_pvtu(directory, name, cnt, nranks, record.fields)
    return piece
