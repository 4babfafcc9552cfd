"""numpy restatement of the splat edits (include/gsplat/gs_abi.h "splat edits"): which splats a filter keeps, in which order,
what an exported record holds, and the columns of a saved .ply.  TEST INFRASTRUCTURE ONLY.

The whole definition: keep = (state & mask) == value; the kept splats come in ascending index order; a record comes back with its
21 padding floats zeroed and every other float as the uploaded bit pattern.  Floats are only ever compared on their uint32 view.
"""
import numpy as np

F = np.float32
HIDDEN, SELECTED = 0x1, 0x2

# The 21 floats of a 320-byte record the device scene does not carry: the fourth lane of the position, the log-scale and the
# opacity vector's tail, and the fourth lane of each of the 16 SH coefficients.
PADDING = [3, 7, 13, 14, 15, 19, 23, 27, 31, 35, 39, 43, 47, 51, 55, 59, 63, 67, 71, 75, 79]
# What gs_repack_kernel reads of a record (k_preprocess.hip): column 0 x y z, column 1 the log-scales, column 2 the rotation,
# column 3 the opacity, columns 4-19 three floats each.
CARRIED = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12] + [16 + 4 * k + c for k in range(16) for c in range(3)]


def keep(state, mask, value):
    return (np.asarray(state, np.uint8).astype(np.uint32) & np.uint32(mask)) == np.uint32(value)


def ids_of(state, mask, value):
    return np.flatnonzero(keep(state, mask, value)).astype(np.uint32)


def zero_padding(rec):
    out = np.array(rec, dtype=F, copy=True).reshape(-1, 80)
    out.view(np.uint32)[:, PADDING] = 0
    return out


def records(rec, state, mask, value):
    return zero_padding(np.asarray(rec, F).reshape(-1, 80)[ids_of(state, mask, value)])


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def sh_rest_count(degree):
    return (degree + 1) ** 2 - 1


def ply_columns(rec, degree):
    """(names, uint32[n, 17 + 3K]): the properties of a saved .ply in file order and the words of every vertex."""
    K = sh_rest_count(degree)
    w = bits(np.asarray(rec, F).reshape(-1, 80))
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    cols = [w[:, 0], w[:, 1], w[:, 2]] + [np.zeros(w.shape[0], np.uint32)] * 3 + [w[:, 16 + c] for c in range(3)]
    for c in range(3):
        for i in range(K):
            names.append("f_rest_%d" % (c * K + i))
            cols.append(w[:, 16 + 4 * (i + 1) + c])
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    cols += [w[:, 12], w[:, 4], w[:, 5], w[:, 6], w[:, 8], w[:, 9], w[:, 10], w[:, 11]]
    return names, np.stack(cols, axis=1) if w.shape[0] else np.zeros((0, len(names)), np.uint32)


def truncate_degree(rec, degree):
    """A record as it reads back from a .ply of that degree: the coefficients above it are zero."""
    out = np.array(rec, dtype=F, copy=True).reshape(-1, 80)
    out.view(np.uint32)[:, 16 + 4 * (degree + 1) ** 2:] = 0
    return out


def parse_ply_header(raw):
    """(vertex count, property names, offset of the vertex data) of a file written by gs_ply_save."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-2] == "end_header" and lines[-1] == ""
    assert lines[2].startswith("element vertex ")
    names = []
    for ln in lines[3:-2]:
        kind, typ, name = ln.split(" ")
        assert kind == "property" and typ == "float"
        names.append(name)
    return int(lines[2].split(" ")[2]), names, end
