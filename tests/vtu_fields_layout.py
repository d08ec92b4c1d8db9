"""The layout rules of an appended-raw `.vtu` piece that carries derived arrays, for a record read by
`tests/vtu_record_reader.read`: the rules of `vtu_record_reader.check_layout` with `vorticity` / `divergence` — one Float64
array of one component each — after `pressure` and before `partitioning`, in that order.

Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

FIELDS = ("vorticity", "divergence")


def check_layout(rec, fields, partitioning=True):
    lay = rec["layout"]
    fields = [f for f in FIELDS if f in fields]
    want = (["points", "velocity", "pressure"] + fields + (["partitioning"] if partitioning else [])
            + ["connectivity", "offsets", "types"])
    assert lay["order"] == want, lay["order"]
    assert lay["contiguous"] and lay["ends_where_the_last_block_says"]
    assert lay["first_block"] % 8 == 0
    n, m = rec["n_points"], rec["n_cells"]
    counts = {name: count for _, name, count in lay["blocks"]}
    assert counts["points"] == 24 * n and counts["velocity"] == 24 * n and counts["pressure"] == 8 * n
    assert all(counts[f] == 8 * n for f in fields)
    assert counts["offsets"] == 4 * m and counts["types"] == m
    assert counts["connectivity"] == 4 * (int(rec["arrays"]["offsets"][-1]) if m else 0)
    types = dict(points="Float64", velocity="Float64", pressure="Float64", connectivity="Int32", offsets="Int32", types="UInt8")
    types.update({f: "Float64" for f in fields})
    if partitioning:
        types["partitioning"] = "Float64"
    assert rec["types"] == types
    assert all(rec["arrays"][f].shape == (n,) for f in fields)
    for off, name, _ in lay["blocks"]:
        if rec["types"][name] == "Float64":
            assert (lay["first_block"] + off + 8) % 8 == 0, name
