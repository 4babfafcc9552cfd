"""A NumPy model of what the tight row pipeline (gaussian-splatting-wgpu_amd/csrc/k_rows.hip) is given and of the tables it builds from
it, for tests/test_row_boundaries.py.  Input: the slot dump of tools/tight_check (run.py dump: gaussian index, slot number, tile row,
first tile column, tiles per slot; tiles == 0 is a hole) and the oracle's depth bucket of every gaussian.  The gaussian-level sort
(k_gsort.hip) orders the gaussians by (bucket, index), as the reference orders a tile's instances; a gaussian's slots stay
consecutive and in slot order.  The row sort partitions the non-hole slots (the items) stably by tile row; a tile row's items are
cut into chunks, and a chunk's items are expanded into instances in item order.

The constants are restated as literals and never read from the library; each names the line it restates.
"""
import numpy as np

SORT_TILE = 4096    # k_rows.hip:39   RA_TILE = RA_THREADS * RA_ITEMS: 8 waves x 64 lanes x 8 slots
SORT_WAVE = 512     # k_rows.hip:120  x0 = s0 + w * (64 * RA_ITEMS): the slots one wave of the row sort takes
GRANULE = 1024      # k_rows.hip:102  chunk_table[s0 >> 10]: one entry of the gaussian sort's chunk table per 1024 slots
LOOKBACK = 8        # k_rows.hip:189  constexpr int LB = 8: predecessors read per round of the look-back
DIGIT_SWITCH = 128  # gs_binning.h:56 gs_digits: 7 bits and hole 127 below 128 tile rows / columns, 8 bits and hole 255 from 128 on
CHUNK = 512         # k_rows.hip:42   RB_CH: items per chunk of count / scan / expansion
SCAN_PARTS = 4      # k_rows.hip:354  per = (nch + 3) / 4: a tile row's chunks in four parts
SCAN_LOADS = 8      # k_rows.hip:357  for (j = j0; j < j1; j += 8): loads per trip of a part
SUB_BATCH = 2048    # k_rows.hip:46   RB_SB: instances per sub-batch of the expansion
EXPAND_WAVE = 512   # k_rows.hip:50   RB_WSL = RB_SB / 4: sub-batch slots of one wave
GRID_UNITS = 4      # gs_frame.hip:73 the row kernels take GS_OPT_PERSISTENT_GRID / 4 as their CU count ...
SORT_WG, COUNT_WG, EXPAND_WG = 3, 8, 6  # k_rows.hip:704, :690, :693 ... and launch 3, 8 and 6 workgroups per CU


def digits(n):
    """(bits, hole digit) for n tile rows or columns."""
    return (7, 127) if n < DIGIT_SWITCH else (8, 255)


def grids(option):
    """Workgroups of the row sort, the count and the expansion under GS_OPT_PERSISTENT_GRID = option."""
    cus = max(option // GRID_UNITS, 1)
    return cus * SORT_WG, cus * COUNT_WG, cus * EXPAND_WG


def _excl(a):
    return np.concatenate([[0], np.cumsum(a)]).astype(np.int64)


def model(slots, bucket):
    """The row pipeline's view of a frame.  Returns a dict:
      S, R, I          slots, items (non-hole slots), instances
      order            the gaussians with slots in depth order (bucket, index)
      first_slot       per entry of `order`: the position of its first slot;  nslots: its slots
      slot_tiles       per slot, in slot order: tiles of the slot (0: hole);  slot_row, slot_col likewise
      tile_valid       per sort tile of SORT_TILE slots: its items
      row_items        [256] items per tile row
      chunks_per_row   [256] ceil(items / CHUNK);  chunk_row, chunk_begin, chunk_end: per chunk its tile row and item range in the
                       row-sorted item array;  chunk_inst: instances per chunk
      item_row, item_col, item_tiles, item_gaussian   the row-sorted items
      item_chunk, item_offset                         per item: its chunk and the instance offset of its first instance inside it
    """
    slots = np.asarray(slots, np.int64).reshape(-1, 5)
    b = np.asarray(bucket, np.int64)[slots[:, 0]]
    o = np.lexsort((slots[:, 1], slots[:, 0], b))
    g, sl, row, col, tiles = (slots[o, k] for k in range(5))
    S = int(g.size)
    head = sl == 0
    order, first_slot = g[head], np.flatnonzero(head)
    nslots = np.diff(np.concatenate([first_slot, [S]]))
    valid = tiles > 0
    tile_valid = np.bincount(np.arange(S)[valid] // SORT_TILE, minlength=-(-S // SORT_TILE)) if S else np.zeros(0, np.int64)
    row_items = np.bincount(row[valid], minlength=256)
    ro = np.argsort(row[valid], kind="stable")
    item_row, item_col, item_tiles, item_g = row[valid][ro], col[valid][ro], tiles[valid][ro], g[valid][ro]
    R = int(item_row.size)
    ibase = _excl(row_items)
    chunks_per_row = -(-row_items // CHUNK)
    cbase = _excl(chunks_per_row)
    chunk_row = np.repeat(np.arange(256), chunks_per_row)
    within = np.arange(chunk_row.size) - cbase[chunk_row]
    chunk_begin = ibase[chunk_row] + within * CHUNK
    chunk_end = np.minimum(chunk_begin + CHUNK, ibase[chunk_row + 1])
    idx = np.arange(R)
    item_chunk = cbase[item_row] + (idx - ibase[item_row]) // CHUNK
    chunk_inst = np.bincount(item_chunk, weights=item_tiles, minlength=chunk_row.size).astype(np.int64)
    before = _excl(item_tiles)[:-1]
    item_offset = before - before[chunk_begin][item_chunk] if R else before
    return {"S": S, "R": R, "I": int(tiles.sum()), "order": order, "first_slot": first_slot, "nslots": nslots, "slot_tiles": tiles,
            "slot_row": row, "slot_col": col, "tile_valid": tile_valid, "row_items": row_items, "chunks_per_row": chunks_per_row,
            "chunk_row": chunk_row, "chunk_begin": chunk_begin, "chunk_end": chunk_end, "chunk_inst": chunk_inst, "item_row": item_row,
            "item_col": item_col, "item_tiles": item_tiles, "item_gaussian": item_g, "item_chunk": item_chunk, "item_offset": item_offset}


def lookback_rounds(tile):
    """Rounds of LOOKBACK predecessors the look-back of sort tile `tile` takes when no predecessor has published its prefix yet."""
    return -(-tile // LOOKBACK)


def scan_parts(nch):
    """Chunks of the four parts of a tile row's scan, and the trips of SCAN_LOADS loads each takes."""
    per = -(-nch // SCAN_PARTS)
    parts = [max(min((p + 1) * per, nch) - min(p * per, nch), 0) for p in range(SCAN_PARTS)]
    return parts, [-(-p // SCAN_LOADS) for p in parts]


def trips(nch, workgroups):
    """Chunks (or sort tiles) each workgroup of a grid-stride loop takes: workgroup w takes w, w + workgroups, ..."""
    return [len(range(w, nch, workgroups)) for w in range(workgroups)]


def straddlers(m, boundary):
    """Indices into m["order"] of the gaussians with a slot on either side of slot `boundary`."""
    return np.flatnonzero((m["first_slot"] < boundary) & (m["first_slot"] + m["nslots"] > boundary))
