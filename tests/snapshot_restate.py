"""numpy restatement of snapshots and write-back (include/gsplat/gs_abi.h "snapshots and write-back").  TEST INFRASTRUCTURE ONLY.

The whole definition: record g of the given records goes to splat ids[g] (ids None: splat g); of it, the floats of the parts named
are copied as words, every other float of the splat, and every other splat, keeps its bit pattern; the state byte of splat ids[g]
becomes states[g] when STATE is named.  What the device holds is what the export restatement returns: the 21 padding floats are
zero whatever was given.  A snapshot is the same write with the records taken earlier.  Floats are only ever compared on their
uint32 view.
"""
import numpy as np

import export_restate as er

F = np.float32
POSITION, GEOMETRY, SH, STATE, RECORD = 0x1, 0x2, 0x4, 0x8, 0x7

# part -> the record floats it names: the floats the device scene carries (export_restate.CARRIED), cut at the record's 16-byte
# vectors -- position (floats 0..3), log-scales, rotation and opacity (4..15), the SH coefficients (16..79)
PART_FLOATS = {POSITION: [f for f in er.CARRIED if f < 4],
               GEOMETRY: [f for f in er.CARRIED if 4 <= f < 16],
               SH: [f for f in er.CARRIED if f >= 16]}
PART_BYTES = {POSITION: 12, GEOMETRY: 32, SH: 192, STATE: 1}
assert sorted(sum(PART_FLOATS.values(), [])) == sorted(er.CARRIED) and not set(er.CARRIED) & set(er.PADDING)
assert all(4 * len(PART_FLOATS[p]) == PART_BYTES[p] for p in PART_FLOATS)


def floats_of(parts):
    """The record floats the parts name, ascending."""
    return sorted(f for p, fl in PART_FLOATS.items() if parts & p for f in fl)


def written(old_records, old_plane, ids, new_records, states, parts):
    """(records, plane) after gs_write_splats(ids, new_records, states, parts) on a context that holds (old_records, old_plane):
    the records as an export of everything returns them."""
    rec = er.zero_padding(old_records)
    plane = None if old_plane is None else np.array(old_plane, dtype=np.uint8, copy=True)
    new = np.ascontiguousarray(new_records, dtype=F).reshape(-1, 80)
    m = new.shape[0]
    at = np.arange(m) if ids is None else np.asarray(ids, np.int64)
    assert at.shape == (m,) and (np.diff(at) > 0).all() and (m == 0 or (at[0] >= 0 and at[-1] < rec.shape[0]))
    fl = floats_of(parts)
    if fl and m:
        rec.view(np.uint32)[np.ix_(at, fl)] = new.view(np.uint32)[:, fl]
    if parts & STATE and m:
        plane[at] = np.asarray(states, np.uint8)
    return rec, plane
