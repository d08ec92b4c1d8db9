"""A reader of `.vtu` pieces, written from the rules of the format, not from the writers.

`read(path)` returns a dict: `n_points`, `n_cells`, `point_data` (the attributes of `<PointData>`), `arrays` (name ->
numpy array; the unnamed array of `<Points>` under "points", with NumberOfComponents > 1 reshaped to [n, components]),
`types` (name -> the `type` attribute) and, for a file with appended data, `layout`: what the checks of the layout need.

ASCII files: every `DataArray` has `format="ascii"` and its numbers as text.  Appended-raw files:
  - `<VTKFile ... byte_order="LittleEndian" header_type="UInt64">`;
  - every `DataArray` carries `format="appended" offset="N"` and no text;
  - after `</UnstructuredGrid>` comes `<AppendedData encoding="raw">`, a newline and a single `_`, then the blocks, then
    `\\n</AppendedData>\\n</VTKFile>\\n`;
  - a block is a UInt64 byte count followed by that many bytes; `offset` counts from the first byte after `_`.
The reader fails (AssertionError) on a file that breaks one of these.

Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import xml.etree.ElementTree as ET

import numpy as np

DTYPES = {"Float64": "<f8", "Int32": "<i4", "UInt8": "u1", "Float32": "<f4", "Int64": "<i8", "UInt64": "<u8"}
OPENING = b'<AppendedData encoding="raw">\n_'
CLOSING = b"\n</AppendedData>\n</VTKFile>\n"


def _shape(a, node):
    nc = int(node.get("NumberOfComponents", "1"))
    return a.reshape(-1, nc) if nc > 1 else a


def _data_arrays(piece):
    out = [("points", piece.find("Points/DataArray"))]
    for group in ("Cells", "PointData"):
        out += [(a.get("Name"), a) for a in piece.find(group)]
    return out


def read(path):
    raw = open(path, "rb").read()
    cut = raw.find(b"<AppendedData")
    if cut < 0:                                                       # an ASCII file
        root = ET.fromstring(raw)
        piece = root.find("UnstructuredGrid/Piece")
        arrays, types = {}, {}
        for name, node in _data_arrays(piece):
            assert node.get("format") == "ascii", name
            types[name] = node.get("type")
            arrays[name] = _shape(np.array(node.text.split(), DTYPES[node.get("type")]), node)
        return dict(n_points=int(piece.get("NumberOfPoints")), n_cells=int(piece.get("NumberOfCells")),
                    point_data=dict(piece.find("PointData").attrib), arrays=arrays, types=types, tokens=_tokens(piece),
                    point_tokens=piece.find("Points/DataArray").text.split())
    # the text before <AppendedData parses as XML once closed
    root = ET.fromstring(raw[:cut] + b"</VTKFile>")
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid" and root.get("version") == "1.0"
    assert root.get("byte_order") == "LittleEndian" and root.get("header_type") == "UInt64"
    assert raw[:cut].rstrip(b" ").endswith(b"</UnstructuredGrid>\n")   # nothing but blanks pads the header
    assert raw[cut:cut + len(OPENING)] == OPENING
    base = cut + len(OPENING)                                         # the first byte after `_`
    piece = root.find("UnstructuredGrid/Piece")
    arrays, types, blocks = {}, {}, []
    for name, node in _data_arrays(piece):
        assert node.get("format") == "appended" and not (node.text or "").strip() and len(node) == 0, name
        o = base + int(node.get("offset"))
        count = int(np.frombuffer(raw, "<u8", 1, o)[0])
        dt = np.dtype(DTYPES[node.get("type")])
        assert count % dt.itemsize == 0 and o + 8 + count <= len(raw), name
        types[name] = node.get("type")
        arrays[name] = _shape(np.frombuffer(raw, dt, count // dt.itemsize, o + 8).copy(), node)
        blocks.append((int(node.get("offset")), name, count))
    blocks.sort()
    end = base + blocks[-1][0] + 8 + blocks[-1][2]                    # where the last block says the data end
    layout = dict(first_block=base, order=[b[1] for b in blocks], blocks=blocks,
                  contiguous=all(a[0] + 8 + a[2] == b[0] for a, b in zip(blocks[:-1], blocks[1:])) and blocks[0][0] == 0,
                  ends_where_the_last_block_says=raw[end:] == CLOSING, size=len(raw))
    return dict(n_points=int(piece.get("NumberOfPoints")), n_cells=int(piece.get("NumberOfCells")),
                point_data=dict(piece.find("PointData").attrib), arrays=arrays, types=types, layout=layout)


def _tokens(piece):
    """The numbers of an ASCII file's point data as the text the writer printed."""
    return {a.get("Name"): a.text.split() for a in piece.find("PointData")}


def check_layout(rec, partitioning=True):
    """The rules an appended-raw file obeys beyond being readable."""
    lay = rec["layout"]
    want = ["points", "velocity", "pressure"] + (["partitioning"] if partitioning else []) + ["connectivity", "offsets", "types"]
    assert lay["order"] == want, lay["order"]
    assert lay["contiguous"] and lay["ends_where_the_last_block_says"]
    assert lay["first_block"] % 8 == 0
    n, m = rec["n_points"], rec["n_cells"]
    counts = {name: count for _, name, count in lay["blocks"]}
    assert counts["points"] == 24 * n and counts["velocity"] == 24 * n and counts["pressure"] == 8 * n
    assert counts["offsets"] == 4 * m and counts["types"] == m
    assert counts["connectivity"] == 4 * (int(rec["arrays"]["offsets"][-1]) if m else 0)
    assert rec["types"] == dict(points="Float64", velocity="Float64", pressure="Float64", connectivity="Int32", offsets="Int32",
                                types="UInt8", **({"partitioning": "Float64"} if partitioning else {}))
    for off, name, _ in lay["blocks"]:
        if rec["types"][name] == "Float64":
            assert (lay["first_block"] + off + 8) % 8 == 0, name
