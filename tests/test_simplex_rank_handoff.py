"""The caller side of the P2/P1 device assembly on several ranks, no GPU: `simplex.device_rank_handoff`,
`force_edges_rank`, `record_points_rank` on the reference's coarse mesh (its cylinder retagged 10, 14 edges) and on
jittered channel meshes, 1 to 4 ranks of `rank_layout` — ranges, closure, and every list against the one-rank list of the
same global block, node or vertex, term for term; the partition that has no closure; the drivers' switch combinations."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from navier_stokes_solver_amd import gmsh as G
from navier_stokes_solver_amd import simplex as SX
from tests.test_simplex import REF_MESH, channel_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = {1: [14], 2: [11, 3], 3: [5, 9, 0], 4: [5, 6, 3, 0]}      # id-10 edges per rank of the cylinder mesh, counted


def cylinder_mesh():
    """The reference's coarse mesh with its interior id-6 segments (the cylinder) tagged 10, as
    tests/test_gpu_forces.py::_cylinder_space does."""
    m = G.read_msh(REF_MESH)
    x = m.nodes[m.lines]
    inside = ((x[:, :, 0] > 1e-9) & (x[:, :, 0] < 2.2 - 1e-9) & (x[:, :, 1] > 1e-9) & (x[:, :, 1] < 0.41 - 1e-9)).all(axis=1)
    return dataclasses.replace(m, line_ids=np.where((m.line_ids == 6) & inside, 10, m.line_ids))


@pytest.fixture(scope="module")
def spaces(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_handoff")
    out = {"cylinder": SX.build_space(cylinder_mesh())}
    for nx, ny in ((4, 3), (10, 5)):
        out[f"channel{nx}x{ny}"] = SX.build_space(G.read_msh(channel_mesh(str(d / f"c{nx}.msh"), nx, ny, jitter=0.25)))
    res = {}
    for name, s in out.items():
        first = SX.assemble(s, 0.1, mode=0, inlet_bc=1, U=0.1)
        res[name] = (s, first, SX.device_handoff(s, first))
    return res


def _lists(ptr, ent, width):
    return [ent[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)], width


@pytest.mark.parametrize("nranks", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh", ["cylinder", "channel4x3", "channel10x5"])
def test_rank_handoff_is_the_one_rank_handoff_term_for_term(spaces, mesh, nranks):
    s, first, one = spaces[mesh]
    lay = SX.rank_layout(s, nranks)
    rp1, col1 = first.F.rowptr.astype(np.int64), first.F.col.astype(np.int64)
    one_blocks = {}                                 # (old row node, old column node) -> the one-rank list as (cell, ln * 6 + lm)
    nblk = (rp1[1::2] - rp1[0:-1:2]) // 2
    b = 0
    for n in range(s.n_un):
        for j in range(int(nblk[n])):
            e = one["blk_ent"][one["blk_ptr"][b]:one["blk_ptr"][b + 1]]
            one_blocks[(n, int(col1[rp1[2 * n] + 2 * j]) // 2)] = [(int(c) // 36, int(c) % 36) for c in e]
            b += 1
    with_pos00, n_edges, own_cells_seen = 0, [], np.zeros(len(s.cell_u), int)
    for r in range(nranks):
        q = SX.local_problem(first, lay, r)
        h = SX.device_rank_handoff(s, lay, r, q)
        n_own, np_own = q.n_u // 2, q.n_p
        n_all, np_all = n_own + len(q.ghost_u) // 2, np_own + len(q.ghost_p)
        cells, T = h["cells"], len(h["cells"])
        if nranks == 1:
            for k in one:
                assert np.array_equal(np.asarray(h[k]), np.asarray(one[k])) and np.asarray(h[k]).dtype == np.asarray(one[k]).dtype, k
        # cells: ascending, the own ones among them, every cell touching an owned node or DoF
        assert (np.diff(cells) > 0).all() and np.array_equal(h["own"], lay.cell_rank[cells] == r)
        assert set(np.nonzero(lay.cell_rank == r)[0]) <= set(cells.tolist())
        # ranges and closure: every node and vertex of a local cell is owned or ghost, and is the node the mesh names
        assert h["cell_u"].shape == (T, 6) and h["cell_u"].min() >= 0 and h["cell_u"].max() < n_all
        assert h["cell_p"].shape == (T, 3) and h["cell_p"].min() >= 0 and h["cell_p"].max() < np_all
        assert np.array_equal(h["node_ids"][h["cell_u"]], s.cell_u[cells]) and np.array_equal(h["vert_ids"][h["cell_p"]], s.cell_p[cells])
        new_of_local = np.concatenate([np.arange(lay.u_ranges[r] // 2, lay.u_ranges[r + 1] // 2), q.ghost_u[0::2] // 2])
        assert np.array_equal(lay.node_new[h["node_ids"]], new_of_local)
        assert np.array_equal(lay.vert_new[h["vert_ids"]], np.concatenate([np.arange(lay.p_ranges[r], lay.p_ranges[r + 1]), q.ghost_p]))
        touching = np.isin(s.cell_u, h["node_ids"][:n_own]).any(axis=1) | np.isin(s.cell_p, h["vert_ids"][:np_own]).any(axis=1)
        assert np.array_equal(np.nonzero(touching | (lay.cell_rank == r))[0], cells)
        assert np.array_equal(h["grad_lam"], s.grad_lam[cells]) and np.array_equal(h["area"], s.area[cells])
        # block lists: positions inside q.F, owned rows; mapped back, the one-rank list of the same global block
        rp, col = q.F.rowptr.astype(np.int64), q.F.col.astype(np.int64)
        assert h["n_blocks"] == len(h["blk_pos0"]) == len(h["blk_pos1"]) == len(h["blk_ptr"]) - 1 == len(col) // 4
        assert h["blk_ptr"][0] == 0 and h["blk_ptr"][-1] == len(h["blk_ent"]) and (np.diff(h["blk_ptr"]) > 0).all()
        assert h["blk_pos0"].min() >= 0 and max(h["blk_pos0"].max(), h["blk_pos1"].max()) + 1 < len(col)
        assert h["blk_ent"].min() >= 0 and h["blk_ent"].max() // 36 < T
        row_of = np.repeat(np.arange(q.n_u), np.diff(rp))
        for bb in range(h["n_blocks"]):
            p0, p1 = int(h["blk_pos0"][bb]), int(h["blk_pos1"][bb])
            n, m = int(row_of[p0]) // 2, int(col[p0]) // 2
            assert row_of[p0] == 2 * n and row_of[p1] == 2 * n + 1 and col[p0 + 1] == col[p0] + 1 and col[p1] == col[p0]
            e = h["blk_ent"][h["blk_ptr"][bb]:h["blk_ptr"][bb + 1]]
            got = [(int(cells[c // 36]), int(c) % 36) for c in e]
            assert got == one_blocks[(int(h["node_ids"][n]), int(h["node_ids"][m]))]
            for c in e:                              # the entry's local nodes are the block's row and column
                assert h["cell_u"][c // 36, (c % 36) // 6] == n and h["cell_u"][c // 36, c % 6] == m
        # node and vertex lists over the owned nodes / DoFs
        for ptr, ent, w, ids, one_ptr, one_ent, n_owned in (
                (h["node_ptr"], h["node_ent"], 6, h["node_ids"], one["node_ptr"], one["node_ent"], n_own),
                (h["vert_ptr"], h["vert_ent"], 3, h["vert_ids"], one["vert_ptr"], one["vert_ent"], np_own)):
            assert len(ptr) == n_owned + 1 and ptr[0] == 0 and ptr[-1] == len(ent) and (np.diff(ptr) > 0).all()
            assert ent.min() >= 0 and ent.max() // w < T
            for i in range(n_owned):
                g = int(ids[i])
                got = [(int(cells[c // w]), int(c) % w) for c in ent[ptr[i]:ptr[i + 1]]]
                assert got == [(int(c) // w, int(c) % w) for c in one_ent[one_ptr[g]:one_ptr[g + 1]]]
        ou = np.stack([2 * h["node_ids"][:n_own], 2 * h["node_ids"][:n_own] + 1], axis=1).reshape(-1)
        assert np.array_equal(h["outlet_w"], one["outlet_w"][ou])
        # pos00: the diagonal entry of the row of OLD DoF 0, on its owner
        if h["pos00"] >= 0:
            with_pos00 += 1
            row = int(row_of[h["pos00"]])
            assert col[h["pos00"]] == row and h["node_ids"][row // 2] == 0 and row % 2 == 0
        else:
            assert h["pos00"] == -1 and not (h["node_ids"][:n_own] == 0).any()
        # the rank's id-10 edges and its piece of the record
        ec, el, nl = SX.force_edges_rank(s, lay, r, h)
        gc, gl, gnl = SX.force_edges(s)
        keep = lay.cell_rank[gc] == r if len(gc) else np.zeros(0, bool)
        assert np.array_equal(cells[ec], gc[keep]) and np.array_equal(el, gl[keep]) and np.array_equal(nl, gnl[keep])
        assert ec.dtype == np.int32 and el.dtype == np.uint8 and h["own"][ec].all()
        n_edges.append(len(ec))
        xy, tris, u_node, p_dof = SX.record_points_rank(s, lay, r, h)
        own = cells[h["own"]]
        verts = h["vert_ids"][p_dof]
        assert np.array_equal(verts, h["node_ids"][u_node]) and len(np.unique(verts)) == len(verts)
        assert set(verts.tolist()) == set(s.cell_p[own].ravel().tolist())            # each own cell's vertices, once
        assert np.array_equal(verts[tris], s.cell_p[own]) and np.array_equal(xy, s.mesh.nodes[verts])
        assert u_node.max() < n_all and p_dof.max() < np_all and u_node.min() >= 0 and p_dof.min() >= 0
        own_cells_seen[own] += 1
    assert with_pos00 == 1 and (own_cells_seen == 1).all()
    if mesh == "cylinder":
        assert n_edges == EDGES[nranks]
        if nranks == 2:
            q0 = SX.local_problem(first, lay, 0)
            h0 = SX.device_rank_handoff(s, lay, 0, q0)
            assert (len(h0["cells"]), int(h0["own"].sum())) == (75, 61)
    else:
        assert sum(n_edges) == 0


def test_an_own_cell_enclosed_by_lower_ranks_is_an_error(spaces):
    s, first, _ = spaces["channel4x3"]
    cell_rank = np.zeros(24, np.int32)
    cell_rank[[13, 23]] = 1
    lay = SX.rank_layout(s, 2, cell_rank=cell_rank)
    assert lay.u_ranges.tolist() == [0, 120, 126] and lay.p_ranges.tolist() == [0, 19, 20]
    SX.device_rank_handoff(s, lay, 0, SX.local_problem(first, lay, 0))             # rank 0 holds everything it needs
    with pytest.raises(ValueError, match=r"cell 13\b"):
        SX.device_rank_handoff(s, lay, 1, SX.local_problem(first, lay, 1))


@pytest.mark.parametrize("driver", ["StationaryNSSolver", "NSSolver"])
def test_device_and_host_assembly_switches_together_end_the_driver(tmp_path, driver):
    """NSK_DEVICE_ASSEMBLY=1 with NSK_HOST_ASSEMBLY=1 on several ranks: one message, status 1, before any handle exists."""
    m = cylinder_mesh()
    path = str(tmp_path / "cyl.msh")
    G.write_msh2(path, m.nodes, m.tris, m.lines, m.line_ids)
    env = dict(os.environ, NSK_OUTPUT_DIR=str(tmp_path), NSK_RANKS="2", NSK_DEVICE_ASSEMBLY="1", NSK_HOST_ASSEMBLY="1",
               NSK_HIP_LIBRARY=str(tmp_path / "no-such-library.so"))                 # (a GPU call would fail on this first)
    args = ["-T", "0.02,0.01"] if driver == "NSSolver" else []
    out = subprocess.run([sys.executable, "-m", "navier_stokes_solver_amd.cli", driver] + args + ["-M", path, "-r", "10", "-p", "2"],
                         capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert out.returncode == 1, (out.stdout[-1000:], out.stderr[-1000:])
    assert out.stderr.count("Error:") == 1 and "NSK_DEVICE_ASSEMBLY=1 does not go with NSK_HOST_ASSEMBLY" in out.stderr
    assert "Number of elements = 122" in out.stdout and not list(tmp_path.glob("*.vtu"))
