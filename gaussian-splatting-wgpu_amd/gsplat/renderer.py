"""Python mirror of the reference's ``Renderer`` (renderer.ts:35-594) on top of the C ABI.

Same constructor shape -- Renderer(canvas, interactiveCamera, device, gaussians, tileSize) -- where
``canvas`` is anything with width/height, ``device`` is a HIP device ordinal and ``gaussians`` has
``numGaussians`` and ``gaussiansBuffer`` (the 320-byte records PackedGaussians builds).
"""
import ctypes
import functools
import inspect

import numpy as np

from . import _abi
from ._abi import GsConfig, GsStats, check


def _sized(call, alloc, dst=lambda out: (out.ctypes.data, len(out))):
    """The C ABI's two-call size protocol.  call(n) reports in n how much there is (bytes or records, as the call counts), alloc(that)
    makes the destination, call(n, *dst(destination)) -- pointer, capacity and what else the call takes -- fills it; the second
    call is left out when there is nothing to fill."""
    n = ctypes.c_uint64()
    check(call(ctypes.byref(n)))
    out = alloc(n.value)
    if n.value:
        check(call(ctypes.byref(n), *dst(out)))
    return out


class Canvas:
    def __init__(self, width, height):
        self.width = int(width)
        self.height = int(height)


class PackedGaussians:
    """Holds the packed 320-byte records (ply.ts:32-47 fields the renderer consumes)."""

    def __init__(self, records):
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
        self.numGaussians = rec.shape[0]
        self.gaussiansBuffer = rec
        self.sphericalHarmonicsDegree = 3


    @staticmethod
    def from_ply(path):
        """Native loader (gs_ply_load): the reference's PackedGaussians(arrayBuffer) for a .ply on disk."""
        rec, deg = _abi.load_ply(path)
        pg = PackedGaussians(rec)
        pg.sphericalHarmonicsDegree = deg
        return pg


class InteractiveCamera:
    """camera.ts:193-308 without the DOM callbacks: dirty flag + camera."""

    def __init__(self, camera):
        self._camera = camera
        self._dirty = True

    def setNewCamera(self, camera):
        self._camera = camera
        self._dirty = True

    def isDirty(self):
        return self._dirty

    def getCamera(self):
        self._dirty = False
        return self._camera


class Renderer:
    def __init__(self, canvas, interactiveCamera, device, gaussians, tileSize=16, *, flags=0, cols=None,
                 max_intersections=0, stream=None, share_with=None):
        """share_with: another Renderer on the same device whose resident splats this one renders (gs_share_splats)
        instead of uploading `gaussians` again."""
        self.canvas = canvas
        self.interactiveCamera = interactiveCamera
        self.device = int(device)
        self.tileSize = int(tileSize)
        self.numGaussians = gaussians.numGaussians
        self.numIntersections = 0
        self.numFrames = 0
        self._L = _abi.load()
        cfg = GsConfig()
        cfg.struct_size = ctypes.sizeof(GsConfig)
        cfg.width, cfg.height, cfg.tile_size = canvas.width, canvas.height, self.tileSize
        cfg.device = self.device
        cfg.col_begin, cfg.col_end = cols if cols is not None else (0, 0)
        cfg.flags = flags
        cfg.max_intersections = int(max_intersections)
        cfg.stream = stream
        self._ctx = ctypes.c_void_p()
        check(self._L.gs_create(ctypes.byref(cfg), ctypes.byref(self._ctx)))
        self.flags = flags
        buf = gaussians.gaussiansBuffer if share_with is None else None
        self._owner = share_with  # keeps the owner of borrowed splats alive
        if share_with is not None:
            check(self._L.gs_share_splats(self._ctx, share_with._ctx))
        elif hasattr(buf, "data_ptr"):  # a device tensor: no PCIe copy
            # the repack runs on the context's stream, which is not ordered against the stream that produced the tensor:
            # the records must be complete before the call (a scene still being generated was repacked half-written when
            # several processes shared one GPU)
            import torch
            torch.cuda.current_stream(buf.device).synchronize()
            check(self._L.gs_upload_splats_device(self._ctx, buf.data_ptr(), self.numGaussians))
        else:
            arr = np.ascontiguousarray(buf, dtype=np.float32)
            check(self._L.gs_upload_splats(self._ctx, arr.ctypes.data, self.numGaussians))
        x0, w = ctypes.c_uint32(), ctypes.c_uint32()
        check(self._L.gs_slab_width(self._ctx, ctypes.byref(x0), ctypes.byref(w)))
        self.slab_x0, self.slab_width = x0.value, w.value

    # -- frame -------------------------------------------------------------------------------------
    def render_uniforms(self, uniforms, debug=False, out_ptr=None):
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(40)
        if out_ptr is not None:
            check(self._L.gs_render_to(self._ctx, u.ctypes.data, out_ptr))
        elif debug:
            check(self._L.gs_render_debug(self._ctx, u.ctypes.data))
        else:
            check(self._L.gs_render(self._ctx, u.ctypes.data))
        self.numFrames += 1

    def animate(self, debug=False):
        """One Renderer.animate() tick (renderer.ts:349-593): renders only when the camera is dirty."""
        if self._ctx is None:
            raise RuntimeError("renderer destroyed")
        if not self.interactiveCamera.isDirty():
            return False
        cam = self.interactiveCamera.getCamera()
        self.render_uniforms(cam.uniforms(self.canvas.width, self.canvas.height), debug=debug)
        return True

    def wait(self):
        check(self._L.gs_wait(self._ctx))

    def set_option(self, key, value):
        check(self._L.gs_set_option(self._ctx, key, int(value)))

    # -- outputs -----------------------------------------------------------------------------------
    def read_rgba8(self):
        out = np.empty((self.canvas.height, self.slab_width, 4), dtype=np.uint8)
        check(self._L.gs_read_rgba8(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def read_buffer(self, which, dtype=np.uint32):
        return _sized(lambda n, dst=None, size=0: self._L.gs_read_buffer(self._ctx, which, dst, size, n),
                      lambda nbytes: np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype),
                      lambda out: (out.ctypes.data, out.nbytes))  # (this call counts bytes)

    def read_alpha(self):
        """GS_FLAG_AUX_OUTPUTS: the last frame's accumulated opacity A = 1 - T, f32[H, slab_width] (0 where no splat reaches).  The
        colour is premultiplied: composite over a background B as C + (1 - A) B."""
        return self.read_buffer(_abi.GS_BUF_ALPHA_F32, np.float32).reshape(self.canvas.height, self.slab_width)

    def read_depth(self, normalized=False):
        """GS_FLAG_AUX_OUTPUTS: the last frame's accumulated depth D = sum of z alpha T (the colour's weights), f32[H, slab_width];
        normalized=True: the expected depth D / A where A > 0, else 0."""
        d = self.read_buffer(_abi.GS_BUF_DEPTH_F32, np.float32).reshape(self.canvas.height, self.slab_width)
        if not normalized:
            return d
        a = self.read_alpha()
        out = np.zeros_like(d)
        np.divide(d, a, out=out, where=a > 0)
        return out

    def pick(self, xy, max_contrib=0):
        """gs_pick: which splats lie under the canvas pixels `xy` (an (n, 2) integer array of x, y) in the last frame.  Returns a
        structured array (_abi.PICK_RESULT_DTYPE: status, list_length, hit_count, first_id / first_depth, max_id / max_weight,
        median_id / median_depth, alpha, depth_acc), one record per query; with max_contrib > 0 also an (n, max_contrib) array of
        the first accepted entries {id, weight} in list order (unused slots {GS_PICK_NONE, 0}).  The answer is the canonical
        (EXACT) blend's, whatever blend the frame used.  At most 65536 queries per call (pick_rect chunks)."""
        q = np.asarray(xy)
        if q.ndim != 2 or q.shape[1] != 2 or q.dtype.kind not in "iu":
            raise ValueError("pick: xy must be an (n, 2) integer array")
        if q.size and q.min() < 0:
            raise ValueError("pick: negative pixel coordinate")
        if q.size and q.max() > 0xFFFFFFFF:
            raise ValueError("pick: pixel coordinate does not fit 32 bits")
        q = np.ascontiguousarray(q, dtype=np.uint32)
        n, mc = q.shape[0], int(max_contrib)
        res = np.zeros(n, dtype=_abi.PICK_RESULT_DTYPE)
        con = np.zeros((n, mc), dtype=_abi.PICK_CONTRIB_DTYPE) if mc else None
        check(self._L.gs_pick(self._ctx, q.ctypes.data if n else None, n, res.ctypes.data if n else None, mc,
                              con.ctypes.data if mc and n else None))
        return (res, con) if mc else res

    def pick_rect(self, x0, y0, x1, y1, which="first"):
        """The rectangle-select of an editor: the sorted unique ids of one field ("first", "max" or "median") over the canvas
        pixels [x0, x1) x [y0, y1), pixels without such a splat (and, on a slab, outside it) left out."""
        if which not in ("first", "max", "median"):
            raise ValueError("pick_rect: which must be first, max or median")
        x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
        if not (0 <= x0 < x1 and 0 <= y0 < y1):
            raise ValueError("pick_rect: empty rectangle")
        w = x1 - x0
        rows = max(1, _abi.GS_PICK_MAX_QUERIES // w)
        ids = [np.zeros(0, np.uint32)]
        for ya in range(y0, y1, rows):
            for xa in range(x0, x1, _abi.GS_PICK_MAX_QUERIES):  # (a row wider than one call is cut too)
                xb, yb = min(x1, xa + _abi.GS_PICK_MAX_QUERIES), min(y1, ya + rows)
                yy, xx = np.meshgrid(np.arange(ya, yb, dtype=np.uint32), np.arange(xa, xb, dtype=np.uint32), indexing="ij")
                r = self.pick(np.stack([xx.ravel(), yy.ravel()], axis=1))
                f = r[which + "_id"][r["status"] == _abi.GS_PICK_OK]
                ids.append(np.unique(f[f != _abi.GS_PICK_NONE]))
        return np.unique(np.concatenate(ids))

    # -- splat state (GS_FLAG_SPLAT_STATE) ------------------------------------------------------------
    def state_region(self, kind, op, bits, where=(0, 0), *, a=(0, 0, 0), b=(0, 0, 0), rect=(0, 0, 0, 0), uniforms=None, mask=None):
        """gs_state_region: applies `op` (GS_STATE_*) with `bits` to every resident splat whose CENTRE lies in the region and
        whose byte passes (s & where[0]) == where[1]; returns how many those are.  kind GS_REGION_SPHERE: a centre, b[0] radius;
        BOX: a min, b max (inclusive); SCREEN_RECT: rect = canvas pixels (x0, y0, x1, y1), half open, under the camera
        `uniforms`; SCREEN_MASK: mask = u8[height, width] of the canvas (nonzero = inside) under `uniforms`; ALL: everything.
        Completes every frame in flight first; the next frame sees the new state."""
        r = _abi.GsRegion()
        r.struct_size, r.kind = ctypes.sizeof(_abi.GsRegion), int(kind)
        r.a[:] = [float(v) for v in a]
        r.b[:] = [float(v) for v in b]
        r.x0, r.y0, r.x1, r.y1 = (int(v) for v in rect)
        u = m = None  # (kept alive until the call returns)
        if uniforms is not None:
            u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(40)
            r.uniforms160 = u.ctypes.data
        if mask is not None:
            m = self._canvas_mask(mask, "state_region")
            r.mask = m.ctypes.data
        r.where_mask, r.where_value = int(where[0]), int(where[1])
        matched = ctypes.c_uint64()
        check(self._L.gs_state_region(self._ctx, ctypes.byref(r), int(op), int(bits), ctypes.byref(matched)))
        return int(matched.value)

    def _canvas_mask(self, mask, who):
        """The mask as the contiguous u8[canvas.height, canvas.width] the C side reads; the caller holds it until its call returns."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (self.canvas.height, self.canvas.width):
            raise ValueError(who + ": the mask must be u8[canvas.height, canvas.width]")
        return m

    def state_ids(self, ids, op, bits):
        """gs_state_ids: the same for a list of splat indices (what pick / pick_rect return); duplicates behave as the sequential
        application would."""
        i = np.asarray(ids)
        if i.size and (i.dtype.kind not in "iu" or i.min() < 0 or i.max() > 0xFFFFFFFF):
            raise ValueError("state_ids: ids must be non-negative 32-bit integers")
        i = np.ascontiguousarray(i, dtype=np.uint32).ravel()
        check(self._L.gs_state_ids(self._ctx, i.ctypes.data if i.size else None, i.size, int(op), int(bits)))

    def state_count(self, mask, value):
        """gs_state_count: splats with (s & mask) == value."""
        n = ctypes.c_uint64()
        check(self._L.gs_state_count(self._ctx, int(mask), int(value), ctypes.byref(n)))
        return int(n.value)

    def read_state(self):
        """The state plane as it is now, u8[N] (GS_BUF_SPLAT_STATE): a snapshot for undo, or a filter over the host's own records."""
        return self.read_buffer(_abi.GS_BUF_SPLAT_STATE, np.uint8)

    def write_state(self, arr):
        """gs_state_write: replaces the whole plane (u8[N]): undo / restore."""
        a = np.ascontiguousarray(arr, dtype=np.uint8).ravel()
        check(self._L.gs_state_write(self._ctx, a.ctypes.data if a.size else None, a.size))

    def select_rect(self, x0, y0, x1, y1, uniforms, op=_abi.GS_STATE_SET):
        return self.state_region(_abi.GS_REGION_SCREEN_RECT, op, _abi.GS_SPLAT_SELECTED, rect=(x0, y0, x1, y1), uniforms=uniforms)

    def select_mask(self, mask, uniforms, op=_abi.GS_STATE_SET):
        return self.state_region(_abi.GS_REGION_SCREEN_MASK, op, _abi.GS_SPLAT_SELECTED, mask=mask, uniforms=uniforms)

    def select_sphere(self, centre, radius, op=_abi.GS_STATE_SET):
        return self.state_region(_abi.GS_REGION_SPHERE, op, _abi.GS_SPLAT_SELECTED, a=centre, b=(radius, 0, 0))

    def select_box(self, lo, hi, op=_abi.GS_STATE_SET):
        return self.state_region(_abi.GS_REGION_BOX, op, _abi.GS_SPLAT_SELECTED, a=lo, b=hi)

    def clear_selection(self):
        return self.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, _abi.GS_SPLAT_SELECTED)

    def hide_selected(self):
        return self.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_SET, _abi.GS_SPLAT_HIDDEN,
                                 where=(_abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_SELECTED))

    def unhide_all(self):
        return self.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, _abi.GS_SPLAT_HIDDEN)

    # -- coverage: per-splat contribution of the last frame, select by what is seen ---------------------------
    def accumulate_coverage(self, rect=None, mask=None):
        """gs_coverage_accumulate: ADDS to this renderer's coverage planes what the last frame shows of the canvas pixels in
        rect = (x0, y0, x1, y1) (half open; None = the whole canvas), optionally AND mask = u8[height, width] of the canvas
        (nonzero = inside): for every pixel and every list entry the blend accepts there, the entry's splat gets hits += 1,
        sum_q += floor(w 2^32) and max_weight = max(max_weight, w), w = alpha T.  Many views, one accumulation.  Returns the
        number of pixels of the region in this renderer's slab (0 when the region misses it)."""
        r = m = None  # (kept alive until the call returns)
        if rect is not None or mask is not None:
            r = _abi.GsCoverRegion()
            r.struct_size = ctypes.sizeof(_abi.GsCoverRegion)
            r.x0, r.y0, r.x1, r.y1 = (int(v) for v in rect) if rect is not None else (0, 0, self.canvas.width, self.canvas.height)
            if mask is not None:
                m = self._canvas_mask(mask, "accumulate_coverage")
                r.mask = m.ctypes.data
        pixels = ctypes.c_uint64()
        check(self._L.gs_coverage_accumulate(self._ctx, ctypes.byref(r) if r is not None else None, ctypes.byref(pixels)))
        return int(pixels.value)

    def reset_coverage(self):
        """gs_coverage_reset: zeroes the coverage planes."""
        check(self._L.gs_coverage_reset(self._ctx))

    def read_coverage(self):
        """gs_coverage_read: the planes as a structured array (_abi.COVERAGE_DTYPE: sum_q, hits, max_weight), one record per
        resident splat; all zero before any accumulate and after an upload or a compaction."""
        return _sized(lambda n, dst=None, cap=0: self._L.gs_coverage_read(self._ctx, dst, cap, n),
                      lambda count: np.zeros(count, dtype=_abi.COVERAGE_DTYPE))

    def state_coverage(self, op, bits, min_hits=1, min_weight=0.0, covered=True, where=(0, 0)):
        """gs_state_coverage: applies `op` (GS_STATE_*) with `bits` to the splats whose byte passes (s & where[0]) == where[1]
        and for which (hits >= min_hits and max_weight >= min_weight) == covered; covered=False names everything NOT seen,
        splats that were never listed included.  Returns how many those are."""
        matched = ctypes.c_uint64()
        check(self._L.gs_state_coverage(self._ctx, int(min_hits), float(min_weight), 1 if covered else 0, int(where[0]), int(where[1]),
                                        int(op), int(bits), ctypes.byref(matched)))
        return int(matched.value)

    def select_visible(self, rect=None, mask=None, min_weight=0.0, op=_abi.GS_STATE_SET):
        """Selects what the last frame SHOWS in the region (not what lies behind it): reset + accumulate + state_coverage on
        GS_SPLAT_SELECTED.  Returns how many splats are covered."""
        self.reset_coverage()
        self.accumulate_coverage(rect, mask)
        return self.state_coverage(op, _abi.GS_SPLAT_SELECTED, 1, min_weight, True)

    def hide_unseen(self, min_hits=1, min_weight=0.0):
        """Hides every splat the accumulated views do not show (floaters behind surfaces, buried interiors); returns their number."""
        return self.state_coverage(_abi.GS_STATE_SET, _abi.GS_SPLAT_HIDDEN, min_hits, min_weight, False)

    # -- splat edits: list, export, compact and save resident splats by state ------------------------------
    def list_state(self, mask, value):
        """gs_state_list: the indices of the splats with (s & mask) == value, ascending, uint32[n]."""
        mask, value = int(mask), int(value)
        return _sized(lambda n, dst=None, cap=0: self._L.gs_state_list(self._ctx, mask, value, dst, cap, n),
                      lambda count: np.empty(count, dtype=np.uint32))

    def export_splats(self, mask=0, value=0, with_ids=False, device=False):
        """gs_export_splats: the resident splats with (s & mask) == value as float32[n, 80] records (what PackedGaussians and the
        uploads take; the 21 padding floats come back 0), in ascending index order.  (0, 0): every splat, also without
        GS_FLAG_SPLAT_STATE.  with_ids: returns (records, uint32[n] old indices).  device=True: torch tensors on this device
        (gs_export_splats_device), never a host copy."""
        mask, value = int(mask), int(value)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            fill, ptr = self._L.gs_export_splats_device, torch.Tensor.data_ptr

            def alloc(m):
                rec = torch.empty((m, 80), dtype=torch.float32, device=dev)
                ids = torch.empty((m,), dtype=torch.int32, device=dev) if with_ids else None
                torch.cuda.current_stream(dev).synchronize()  # the allocator may hand out memory another stream still uses
                return rec, ids
        else:
            fill, ptr = self._L.gs_export_splats, lambda a: a.ctypes.data

            def alloc(m):
                return np.empty((m, 80), dtype=np.float32), np.empty(m, dtype=np.uint32) if with_ids else None

        def call(n, dst=None, cap=0, dst_ids=None):  # (the size is asked of gs_export_splats on either path)
            return (fill if dst else self._L.gs_export_splats)(self._ctx, mask, value, dst, cap, n, dst_ids)
        rec, ids = _sized(call, alloc, lambda out: (ptr(out[0]), len(out[0]), ptr(out[1]) if with_ids else None))
        return (rec, ids) if with_ids else rec

    def compact(self, mask, value):
        """gs_compact: keeps the splats with (s & mask) == value, drops the rest for good and renumbers.  Returns the id map
        uint32[kept]: ids[new index] = old index (how a host renumbers its own per-splat metadata).  State bytes are carried;
        the next frame renders what the scene with the dropped splats hidden rendered.  Like an upload, taps and pick need a
        new frame afterwards."""
        st = GsStats()
        check(self._L.gs_get_stats(self._ctx, ctypes.byref(st)))  # N before the call: the capacity gs_compact expects of ids
        ids = np.empty(max(int(st.num_gaussians), 1), dtype=np.uint32)
        kept = ctypes.c_uint64()
        check(self._L.gs_compact(self._ctx, int(mask), int(value), ctypes.byref(kept), ids.ctypes.data))
        self.numGaussians = int(kept.value)
        return ids[:self.numGaussians].copy()

    def delete_hidden(self):
        """Removes every hidden splat for good (compact(GS_SPLAT_HIDDEN, 0)); returns the id map."""
        return self.compact(_abi.GS_SPLAT_HIDDEN, 0)

    def save_ply(self, path, mask=0, value=0, sh_degree=3):
        """gs_export_ply: streams the splats with (s & mask) == value into a binary 3DGS .ply (no whole-scene host buffer);
        returns how many were written."""
        n = ctypes.c_uint64()
        check(self._L.gs_export_ply(self._ctx, str(path).encode(), int(mask), int(value), int(sh_degree), ctypes.byref(n)))
        return int(n.value)

    # -- splat transforms: move, rotate and scale resident splats in place ----------------------------------
    def transform(self, xform, mask=_abi.GS_SPLAT_SELECTED, value=_abi.GS_SPLAT_SELECTED):
        """gs_transform_splats: applies a GsXform (_abi.compose_xform) in place to the resident splats with (s & mask) == value
        (default: the selection; (0, 0): every splat, also without GS_FLAG_SPLAT_STATE); returns how many those are.  Completes
        every frame in flight first; not a frame and not an upload: the next frame sees the moved splats.  The inverse transform
        is not a bit-exact undo: export the selection first if one is needed."""
        matched = ctypes.c_uint64()
        check(self._L.gs_transform_splats(self._ctx, int(mask), int(value), ctypes.byref(xform), ctypes.byref(matched)))
        return int(matched.value)

    def translate_selected(self, t):
        return self.transform(_abi.compose_xform(translate=t))

    def rotate_selected(self, rot, pivot=None):
        """rot: quaternion (r, x, y, z) of any non-zero length; pivot: the point that stays where it is (default: the origin)."""
        return self.transform(_abi.compose_xform(rot=rot, pivot=pivot))

    def scale_selected(self, s, pivot=None):
        return self.transform(_abi.compose_xform(scale=s, pivot=pivot))

    def device_ptr(self, which):
        p = ctypes.c_void_p()
        check(self._L.gs_device_ptr(self._ctx, which, ctypes.byref(p)))
        return p.value

    def stats(self):
        s = GsStats()
        check(self._L.gs_get_stats(self._ctx, ctypes.byref(s)))
        d = {k: getattr(s, k) for k, t in GsStats._fields_ if not issubclass(t, ctypes.Array)}  # (the two arrays go in by stage name)
        d["stage_us"] = {n: s.stage_us[i] for i, n in enumerate(_abi.GS_STAGE_NAMES)}
        d["stage_us_mean"] = {n: s.stage_us_mean[i] for i, n in enumerate(_abi.GS_STAGE_NAMES)}
        self.numIntersections = d["num_intersections"]
        return d

    def assemble(self, d_slabs_ptr, col_bounds, slab_stride_bytes, d_image_ptr):
        cb = (ctypes.c_uint32 * len(col_bounds))(*col_bounds)
        check(self._L.gs_assemble_slabs(self._ctx, d_slabs_ptr, cb, len(col_bounds) - 1, slab_stride_bytes, d_image_ptr))

    def destroy(self):
        """Renderer.destroy (renderer.ts:90-94); safe to call twice and before the first frame."""
        if self._ctx is not None:
            check(self._L.gs_destroy(self._ctx))
            self._ctx = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PipelinedRenderer:
    """K frames in flight: K contexts (one uploads the splats, the others borrow them) rendered round-robin, each on its
    own stream with its own per-frame buffers, so frame k's blend overlaps frame k+1's binning and sort.  The reference
    keeps one frame in flight (Renderer.animate awaits every stage, renderer.ts:394-587); results per frame are identical.
    `render_uniforms` returns the slot used; `wait(slot)` / `read_rgba8(slot)` address a frame; `wait()` drains all."""

    def __init__(self, canvas, interactiveCamera, device, gaussians, tileSize=16, *, frames_in_flight=2, **kw):
        if frames_in_flight < 1:
            raise ValueError("frames_in_flight must be >= 1")
        first = Renderer(canvas, interactiveCamera, device, gaussians, tileSize, **kw)
        self.renderers = [first] + [Renderer(canvas, interactiveCamera, device, gaussians, tileSize, share_with=first, **kw)
                                    for _ in range(frames_in_flight - 1)]
        for r in self.renderers:  # this class IS the explicit form of the library's own ring: its members render one frame at a time
            r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        self.canvas, self.interactiveCamera = canvas, interactiveCamera
        self._next = 0
        self._busy = [False] * frames_in_flight
        self.numFrames = 0

    def render_uniforms(self, uniforms):
        slot = self._next
        r = self.renderers[slot]
        if self._busy[slot]:
            r.wait()  # the frame this context rendered K steps ago must be complete before its buffers are reused
        r.render_uniforms(uniforms)
        self._busy[slot] = True
        self._next = (slot + 1) % len(self.renderers)
        self.numFrames += 1
        return slot

    def animate(self):
        if not self.interactiveCamera.isDirty():
            return None
        cam = self.interactiveCamera.getCamera()
        return self.render_uniforms(cam.uniforms(self.canvas.width, self.canvas.height))

    def wait(self, slot=None):
        for k, r in enumerate(self.renderers):
            if (slot is None or slot == k) and self._busy[k]:
                r.wait()
                self._busy[k] = False

    def set_option(self, key, value):
        for r in self.renderers:
            r.set_option(key, value)

    # splat state: the plane lives with the owner's splats, the borrowers render it.  Their frames are the host's to drain
    # (gs_abi.h): every slot is drained here, then the owner is asked
    def _state_owner(self):
        self.wait()
        return self.renderers[0]

    # coverage: the planes are the owner's, and so is the frame they describe (slot 0's last one).  Splat edits and transforms go to
    # the owner too; after a compaction the other members borrow the new scene, as the constructor made them (compact, below)
    _OWNER_CALLS = ("state_region", "state_ids", "state_count", "read_state", "write_state", "select_rect", "select_mask", "select_sphere",
                    "select_box", "clear_selection", "hide_selected", "unhide_all",
                    "accumulate_coverage", "reset_coverage", "read_coverage", "state_coverage", "select_visible", "hide_unseen",
                    "list_state", "export_splats", "save_ply", "transform", "translate_selected", "rotate_selected", "scale_selected")
    # per-frame outputs: `slot` (what render_uniforms returned) comes first, the slot's frame is waited for, its renderer answers
    _SLOT_CALLS = ("read_rgba8", "read_alpha", "read_depth", "pick")

    def _owner_call(name):
        @functools.wraps(getattr(Renderer, name))
        def call(self, *a, **kw):
            return getattr(self._state_owner(), name)(*a, **kw)
        return call

    def _slot_call(name):
        @functools.wraps(getattr(Renderer, name))
        def call(self, slot, *a, **kw):
            self.wait(slot)
            return getattr(self.renderers[slot], name)(*a, **kw)
        own, *rest = inspect.signature(call).parameters.values()  # (Renderer's parameters: `slot` goes in behind self)
        call.__signature__ = inspect.Signature([own, inspect.Parameter("slot", inspect.Parameter.POSITIONAL_OR_KEYWORD)] + rest)
        return call

    for _name in _OWNER_CALLS:  # (plain functions while the class body runs; the methods they make are ordinary class attributes)
        locals()[_name] = _owner_call(_name)
    for _name in _SLOT_CALLS:
        locals()[_name] = _slot_call(_name)
    del _name, _owner_call, _slot_call

    def compact(self, mask, value):
        first = self._state_owner()
        ids = first.compact(mask, value)
        for r in self.renderers[1:]:
            check(r._L.gs_share_splats(r._ctx, first._ctx))
            r.numGaussians = first.numGaussians
        return ids

    def delete_hidden(self):
        return self.compact(_abi.GS_SPLAT_HIDDEN, 0)

    def destroy(self):
        for r in reversed(self.renderers):  # borrowers first
            r.destroy()
