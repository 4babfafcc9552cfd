"""A NumPy restatement of the bookkeeping of the tight projection (gaussian-splatting-wgpu_amd/csrc/k_preprocess.hip,
gs_preprocess_kernel<TIGHT = true, NB, STATE>), for tests/test_projection_slots.py.  Input: the slots of every splat (the dump of
tools/tight_check through row_scenes.per_splat; 0 for a survivor that ends without a tile), the cull mask AS THE SCENE BUILDER MADE IT
(a splat centred inside the canvas survives, one centred at ndc x >= 5 is culled: the frustum test is not re-derived here), NB and n.

A workgroup covers indices [512 NB b, 512 NB (b + 1)); its survivors are compacted in index order; survivor v is lane v % 64 of wave
(v / 64) % 4 of trip v / 256.  The constants are restated as literals and never read from the library; each names what it restates.
"""
import numpy as np

CHUNK = 512       # k_preprocess.hip PRE_G: gaussians per cull chunk; a workgroup takes NB of them
TRIP = 256        # one survivor per thread and trip
WAVE = 64
UNIT = 1024       # consecutive indices whose survivors share a run of entries (two cull chunks)
SHARDS = 16       # bump cursors of each kind: shard = workgroup & 15
MAX_SLOTS = 2 * 255  # of one splat: 255 tile rows, twice with the aliased column
FRESH_ROWS = 1 << 20  # gs_context.hip: a fresh context's arena holds max(2 n, 2^20) slots


def shard_cap(row_capacity):
    """Arena slots of one shard (k_preprocess.hip: shard_cap = f.row_cap >> 4)."""
    return row_capacity >> 4


def rec_shard_cap(n, NB):
    """Record slots of one shard (gs_preprocess_prepare: ceil(workgroups / 16) * 512 * NB)."""
    wgs = -(-n // (CHUNK * NB))
    return -(-wgs // SHARDS) * CHUNK * NB


def fits(at, R, cap, strict=True):
    """The kernel's fit test of a bump of R slots at cursor value `at` (`at > cap || R > cap - at` refuses); strict=False restates it
    with >= in place of >, which refuses a bump that ends exactly on the shard's last slot."""
    return not (at > cap or R > cap - at) if strict else not (at >= cap or R >= cap - at)


def model(nslots, culled, NB, n=None):
    """Per workgroup b a dict:
      survivors   indices in index order;  nvis, trips
      ns, valid   [trips, 4, 64] slots of the survivor in (trip, wave, lane) (0 where valid is False: an idle lane replays survivor
                  nvis - 1 and has no slots of its own);  myrp: its first slot inside the wave's
      Rw, Cw      [trips, 4] slots of the wave, survivors with slots;  word = Rw | Cw << 16 (s_tw)
      R, C        [trips] the trip's bumps of the row and the record cursor (no bump when R == 0)
      entry       per survivor, the kernel's way: ((b * (NB / 2) + uk) << 10) + (v - first survivor of unit uk)
      entry_direct  unit * 1024 + rank among the unit's survivors
    and for the frame: unit_n [ceil(n / 1024)], shard_rows [16], shard_recs [16], workgroups."""
    nslots = np.asarray(nslots, np.int64)
    culled = np.asarray(culled, bool)
    n = nslots.size if n is None else n
    assert nslots.size == n == culled.size and (nslots[culled] == 0).all() and nslots.max(initial=0) <= MAX_SLOTS
    G = CHUNK * NB
    nwg = -(-n // G)
    units = -(-n // UNIT)
    unit_n = np.bincount(np.flatnonzero(~culled) // UNIT, minlength=units)
    shard_rows, shard_recs = np.zeros(SHARDS, np.int64), np.zeros(SHARDS, np.int64)
    wgs = []
    for b in range(nwg):
        idx = np.arange(b * G, min((b + 1) * G, n))
        surv = idx[~culled[idx]]
        nvis = surv.size
        trips = -(-nvis // TRIP)
        ns = np.zeros(trips * TRIP, np.int64)
        ns[:nvis] = nslots[surv]
        valid = np.arange(trips * TRIP) < nvis
        ns, valid = ns.reshape(trips, 4, WAVE), valid.reshape(trips, 4, WAVE)
        incl = np.cumsum(ns, axis=2)
        Rw, Cw = incl[:, :, -1], (ns > 0).sum(axis=2)
        R, C = Rw.sum(axis=1), Cw.sum(axis=1)
        # entries: rounds 4 uk .. 4 uk + 3 of the cull (256 indices each) are unit uk of the workgroup
        uk = (surv - b * G) >> 10
        first = np.array([int((uk < k).sum()) for k in range(NB // 2)], np.int64)  # s_ust
        v = np.arange(nvis)
        entry = ((b * (NB // 2) + uk) << 10) + (v - (0 if NB == 2 else first[uk]))
        unit = surv // UNIT
        rank = v - np.searchsorted(unit, unit, "left")
        shard_rows[b % SHARDS] += R.sum()
        shard_recs[b % SHARDS] += C.sum()
        wgs.append(dict(survivors=surv, nvis=nvis, trips=trips, ns=ns, valid=valid, myrp=incl - ns, Rw=Rw, Cw=Cw, word=Rw | (Cw << 16),
                        R=R, C=C, entry=entry, entry_direct=unit * UNIT + rank, unit=unit, first=first))
    return dict(wg=wgs, unit_n=unit_n, shard_rows=shard_rows, shard_recs=shard_recs, workgroups=nwg, NB=NB, n=n)


# ---- the owner of every (wave, batch, lane) of one trip ------------------------------------------------------------------------------
def owners_direct(ns):
    """ns [4, 64] -> per wave an array [Rw]: the lane whose [myrp, myrp + nslots) holds the slot."""
    out = []
    for w in range(4):
        incl = np.cumsum(ns[w])
        out.append(np.searchsorted(incl, np.arange(int(incl[-1])), "right"))
    return out


def owners_kernel(ns, carry=True, strict=True, empty_marks=False):
    """The kernel's way, on a restated s_mark of the trip's 256 threads: per batch of 64 slots every wave that still has slots clears
    its 64 words, every survivor with slots whose first slot lies in the batch stores lane + 1 at that position, an inclusive running
    maximum spreads the marks and is joined (max) with the carry of the previous batch.  carry=False drops the carry; strict=False
    tests the mark's position with <= instead of <, so that a first slot at the NEXT batch's position 0 is also stored at position 64
    of this one -- the next wave's word 0 (beyond the array for wave 3).  The waves are taken in lockstep and such a stray store lands
    after the owner's own (what the hardware does with the two stores is not defined; the restatement takes the order that shows).
    empty_marks=True drops the `nslots &&` of the mark test: a lane without slots stores too, at the position of the next survivor
    with slots, and of the lanes that store to one word the lowest lands last (again the order that shows).
    Returns (owners per wave [Rw] as lanes, -1 where no owner was found; mark-less batches per wave)."""
    ns = np.asarray(ns, np.int64)
    incl = np.cumsum(ns, axis=1)
    myrp, Rw = incl - ns, incl[:, -1]
    own = [np.full(int(Rw[w]), -1, np.int64) for w in range(4)]
    markless = [0, 0, 0, 0]
    jc = [0, 0, 0, 0]
    for rb0 in range(0, int(Rw.max(initial=0)), WAVE):
        mark = np.zeros(4 * WAVE + 1, np.int64)
        stray = []
        live = [w for w in range(4) if rb0 < Rw[w]]
        for w in live:
            hi = rb0 + WAVE
            has = (ns[w] > 0) | empty_marks
            for lane in np.flatnonzero(has & (myrp[w] >= rb0) & ((myrp[w] < hi) if strict else (myrp[w] <= hi)))[::-1 if empty_marks else 1]:
                pos = int(myrp[w][lane]) - rb0
                if pos == WAVE:
                    stray.append((min(WAVE * (w + 1), 4 * WAVE), lane + 1))
                else:
                    mark[WAVE * w + pos] = lane + 1
        for at, val in stray:
            mark[at] = val
        for w in live:
            mk = mark[WAVE * w:WAVE * (w + 1)]
            if not mk.any():
                markless[w] += 1
            m = np.maximum.accumulate(mk)
            if carry:
                m = np.maximum(m, jc[w])
                jc[w] = int(m[-1])
            k = min(WAVE, int(Rw[w]) - rb0)
            own[w][rb0:rb0 + k] = m[:k] - 1
    return own, markless
