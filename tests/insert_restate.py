"""numpy restatement of the splat insertion (include/gsplat/gs_abi.h "splat insertion"): what a context holds after an append or a
duplicate.  TEST INFRASTRUCTURE ONLY.

The whole definition: the records are the old ones followed by the new ones, with the 21 padding floats as +0 (export_restate's
rule: the device scene does not carry them); the state plane is the old bytes followed by m times new_state; a duplicate's new
records are the old records of the ascending matches of its filter.  Floats are only ever compared on their uint32 view.
"""
import numpy as np

import export_restate as er

F = np.float32


def appended(old_rec, old_state, new_rec, new_state):
    """(records float32[N + m, 80], state uint8[N + m], first, count) after an append of new_rec with the byte new_state."""
    old = np.asarray(old_rec, F).reshape(-1, 80)
    new = np.asarray(new_rec, F).reshape(-1, 80)
    rec = er.zero_padding(np.concatenate([old, new]))
    state = np.concatenate([np.asarray(old_state, np.uint8).ravel(), np.full(new.shape[0], new_state, np.uint8)])
    return rec, state, old.shape[0], new.shape[0]


def duplicated(old_rec, old_state, mask, value, new_state):
    """The same after a duplicate of the splats with (s & mask) == value, and the source ids (ascending)."""
    ids = er.ids_of(old_state, mask, value)
    rec, state, first, count = appended(old_rec, old_state, np.asarray(old_rec, F).reshape(-1, 80)[ids], new_state)
    return rec, state, first, count, ids
