'use strict';
// Node-host restatement of the reference's Renderer (renderer.ts:35-594) on the MI355X C ABI.
// Same constructor and methods: new Renderer(canvas, interactiveCamera, device, gaussians, tileSize),
// animate(): Promise<void>, destroy(): Promise<void>.  `canvas` is any {width, height} with an
// optional onFrame(Uint8Array rgba, width, height) sink (the blit target of render.wgsl);
// `device` is the HIP device ordinal (or {ordinal, flags}) where the reference takes a GPUDevice.
const path = require('path');

let native = null;
function loadNative() {
  if (!native) {
    const file = path.join(__dirname, '..', 'lib', 'gsplat_napi.node');
    try {
      native = require(file);
    } catch (e) {
      throw new Error(`gsplat: native addon not built (${file}): run python gaussian-splatting-wgpu_amd/csrc/build.py; there is no fallback renderer. ${e.message}`);
    }
  }
  return native;
}

class Renderer {
  constructor(canvas, interactiveCamera, device, gaussians, tileSize) {
    this.tileSize = tileSize;
    this.canvas = canvas;
    this.interactiveCamera = interactiveCamera;
    this.device = device;
    this.numFrames = 0;
    this.numIntersections = 0;
    this.numGaussians = gaussians.numGaussians;
    this.destroyCallback = null;
    this.destroyed = false;
    this.lastDraw = Date.now();
    this.frameTimes = null;
    const n = loadNative();
    const ordinal = typeof device === 'number' ? device : ((device && device.ordinal) || 0);
    const flags = (device && device.flags) || 0;
    // device.shareWith: another Renderer on the same device whose resident splats this one renders (gs_share_splats) -
    // several renderers driven round-robin keep several frames in flight (the reference has one: every stage is awaited)
    const owner = (device && device.shareWith) || null;
    this.owner = owner; // keeps the owner alive
    if (!canvas || !(canvas.width > 0) || !(canvas.height > 0)) throw new Error('WebGPU context not found!'); // renderer.ts:108-111
    this.handle = n.create({ width: canvas.width, height: canvas.height, tileSize, device: ordinal, flags });
    if (owner) n.shareSplats(this.handle, owner.handle);
    else if (gaussians.plyPath) this.numGaussians = n.uploadPly(this.handle, gaussians.plyPath); // streaming loader: no packed buffer on the host
    else n.uploadSplats(this.handle, gaussians.gaussiansBuffer, this.numGaussians); // renderer.ts:130-137
    this.uniforms = new Float32Array(40);
    // canvas.pipeline = K >= 2 (extension; the reference awaits every stage of every frame, renderer.ts:394-587): animate() still
    // resolves once per frame and hands onFrame that frame's pixels, but it enqueues frame k+1 before frame k's pixels have
    // arrived -- up to K frames are on the device at once -- and the pixels land in K page-locked sinks that are reused
    // (a view handed to onFrame is valid until K more frames have been enqueued) instead of a fresh 8 MB ArrayBuffer per frame.
    this.pipeline = Math.max(1, Math.min(4, (canvas.pipeline | 0) || 1));
    this.sinks = null;
    this.pending = []; // promises of the frames in flight, oldest first
    this.slot = 0;
    if (this.pipeline > 1) {
      const bytes = canvas.width * canvas.height * 4;
      this.sinks = [];
      for (let k = 0; k < this.pipeline; ++k) this.sinks.push(new Uint8Array(n.hostAlloc(bytes)));
    }
    this.autoSchedule = !(canvas.manual === true);
    if (this.autoSchedule) setImmediate(() => this.animate()); // requestAnimationFrame(() => this.animate()), renderer.ts:323
  }

  // resolves when the renderer has been torn down on the next animate() tick (renderer.ts:90-94)
  destroy() {
    return new Promise((resolve) => {
      this.destroyCallback = resolve;
      if (!this.autoSchedule) this.animate();
    });
  }

  destroyImpl() {
    if (this.destroyCallback === null) throw new Error('destroyImpl called without destroyCallback set!');
    if (!this.destroyed) {
      loadNative().destroy(this.handle); // (frames still in flight: the native side defers the teardown to their completion)
      this.destroyed = true;
    }
    this.destroyCallback();
  }

  // One frame of the pipelined mode: enqueue now, resolve when THIS frame's pixels are in its sink.
  animatePipelined() {
    const n = loadNative();
    const k = this.slot;
    this.slot = (k + 1) % this.pipeline;
    const sink = this.sinks[k];
    const u = new Float32Array(this.uniforms); // this frame's block: `uniforms` is repacked by the next animate() before the enqueue below may run
    const wait = this.pending.length >= this.pipeline ? this.pending.shift() : Promise.resolve();
    // the sink of slot k is free once the frame that used it K frames ago has been delivered
    const p = wait.then(() => {
      if (this.destroyed) return undefined;
      return n.renderToSink(this.handle, u, sink).then(() => {
        this.numFrames++;
        if (typeof this.canvas.onFrame === 'function') this.canvas.onFrame(sink, this.canvas.width, this.canvas.height);
      });
    });
    this.pending.push(p.catch(() => {}));
    return p;
  }

  async animate() {
    if (this.destroyCallback !== null) {
      if (this.pending.length) { await Promise.all(this.pending); this.pending = []; }
      this.destroyImpl();
      return;
    }
    if (this.destroyed) return;
    const rearm = () => { if (this.autoSchedule) setImmediate(() => this.animate()); };
    if (!this.interactiveCamera.isDirty()) { rearm(); return; }
    const camera = this.interactiveCamera.getCamera();
    camera.packUniforms(this.canvas.width, this.canvas.height, this.uniforms); // renderer.ts:362-392
    if (this.pipeline > 1) {
      const p = this.animatePipelined(); // (the uniforms are copied by the native call before it returns)
      rearm(); // the next frame may be enqueued at once
      await p;
      return;
    }
    const n = loadNative();
    await n.renderAsync(this.handle, this.uniforms); // the whole frame, renderer.ts:394-574
    if (this.destroyed) return;
    const st = n.stats(this.handle);
    this.numIntersections = st.numIntersections;
    this.frameTimes = st.stageUs;
    this.numFrames++;
    if (typeof this.canvas.onFrame === 'function') {
      this.canvas.onFrame(new Uint8Array(n.readRgba8(this.handle)), this.canvas.width, this.canvas.height);
    }
    rearm();
  }

  // synchronous helpers for tools and tests
  renderUniforms(uniforms, debug) { loadNative().renderSync(this.handle, uniforms, !!debug); this.numFrames++; }
  readPixels() { return new Uint8Array(loadNative().readRgba8(this.handle)); }
  readBuffer(which) { return loadNative().readBuffer(this.handle, which); }
  // GS_FLAG_AUX_OUTPUTS ({ordinal, flags} at construction): the last frame's f32[height][slabWidth] planes.  readAlpha(): accumulated
  // opacity A (the colour is premultiplied: C + (1 - A) * background); readDepth(): accumulated depth D, or with normalized = true
  // the expected depth D / A where A > 0 (0 elsewhere)
  readAlpha() { const n = loadNative(); return new Float32Array(n.readBuffer(this.handle, n.BUF_ALPHA_F32)); }
  readDepth(normalized) {
    const n = loadNative();
    const d = new Float32Array(n.readBuffer(this.handle, n.BUF_DEPTH_F32));
    if (!normalized) return d;
    const a = this.readAlpha();
    for (let i = 0; i < d.length; ++i) d[i] = a[i] > 0 ? d[i] / a[i] : 0;
    return d;
  }
  // gs_pick: which splats lie under canvas pixels of the last frame.  queries: Uint32Array of x,y pairs (at most 65536 pairs per call);
  // maxContrib > 0 also returns the first accepted entries of every pixel.  The result holds typed-array views over the native
  // 48-byte records (u32 and f32 share the bytes: word 12 q + k, see FIELD) and get(q), which decodes one record.
  pick(queries, maxContrib = 0) {
    if (!(queries instanceof Uint32Array) || queries.length % 2 !== 0) throw new TypeError('gsplat: pick expects a Uint32Array of x,y pairs');
    const n = loadNative();
    const raw = n.pick(this.handle, queries, maxContrib >>> 0);
    return new PickResult(raw.results, raw.contrib, queries.length / 2, maxContrib >>> 0);
  }
  stats() { return loadNative().stats(this.handle); }
  setOption(key, value) { loadNative().setOption(this.handle, key, value); }
  // Splat state (FLAG.SPLAT_STATE at construction): one byte per resident splat -- STATE.HIDDEN splats are not rendered, STATE.SELECTED
  // ones are drawn tinted (setOption(OPT.SELECT_TINT, a<<24 | r<<16 | g<<8 | b)), bits 2-7 are the host's.  Every call completes the
  // frames in flight first; the next frame sees the new state.
  // stateRegion({kind: REGION.*, a, b, x0, y0, x1, y1, uniforms, mask, whereMask, whereValue}, op, bits) -> splats matched: `op`
  // (STATE.SET / CLEAR / TOGGLE / ASSIGN) is applied to every splat whose CENTRE lies in the region and whose byte passes
  // (s & whereMask) == whereValue.  SPHERE: a centre, b[0] radius; BOX: a min, b max; SCREEN_RECT: canvas pixels [x0,x1) x [y0,y1)
  // under the camera `uniforms`; SCREEN_MASK: mask = Uint8Array[height * width] of the canvas, nonzero = inside.
  stateRegion(region, op, bits) {
    const r = Object.assign({}, region);
    if (r.mask) { r.maskWidth = this.canvas.width; r.maskHeight = this.canvas.height; }
    return loadNative().stateRegion(this.handle, r, op >>> 0, bits >>> 0);
  }
  // the same for a Uint32Array of splat indices (what pick returns); duplicates behave as the sequential application would
  stateIds(ids, op, bits) {
    if (!(ids instanceof Uint32Array)) throw new TypeError('gsplat: stateIds expects a Uint32Array of splat indices');
    loadNative().stateIds(this.handle, ids, op >>> 0, bits >>> 0);
  }
  stateCount(mask, value) { return loadNative().stateCount(this.handle, mask >>> 0, value >>> 0); }
  readState() { return new Uint8Array(loadNative().readState(this.handle)); } // the plane as it is now: undo snapshot, export filter
  writeState(bytes) {
    if (!(bytes instanceof Uint8Array)) throw new TypeError('gsplat: writeState expects a Uint8Array of N state bytes');
    loadNative().writeState(this.handle, bytes);
  }
  // Coverage: which splats the last frame actually SHOWS.  accumulateCoverage({x0, y0, x1, y1, mask}) ADDS, for every canvas pixel of
  // the rect (null: the whole canvas; mask: Uint8Array[height * width] of the canvas, nonzero = inside) and every list entry the blend
  // accepts there, hits += 1, sumQ += floor(w 2^32) and maxWeight = max(maxWeight, w) to the record of the entry's splat (w = alpha T);
  // returns the pixels of the region in this renderer's slab.  Many views, one accumulation; an upload or a compaction drops the planes.
  accumulateCoverage(region = null) {
    let r = null;
    if (region) {
      r = Object.assign({ x0: 0, y0: 0, x1: this.canvas.width, y1: this.canvas.height }, region);
      if (r.mask) {
        if (!(r.mask instanceof Uint8Array)) throw new TypeError('gsplat: accumulateCoverage expects mask to be a Uint8Array');
        r.maskWidth = this.canvas.width; r.maskHeight = this.canvas.height;
      }
    }
    return loadNative().accumulateCoverage(this.handle, r);
  }
  resetCoverage() { loadNative().resetCoverage(this.handle); }
  // -> {count, bytes, u64, u32, f32}: count records of 16 bytes (gs_coverage_rec) and typed-array views over them, record i at
  // u64[2 i + COVERAGE_FIELD.sumQ / 8], u32[4 i + COVERAGE_FIELD.hits / 4], f32[4 i + COVERAGE_FIELD.maxWeight / 4]
  readCoverage() {
    const bytes = loadNative().readCoverage(this.handle);
    return { count: bytes.byteLength / COVERAGE.REC_BYTES, bytes, u64: new BigUint64Array(bytes), u32: new Uint32Array(bytes), f32: new Float32Array(bytes) };
  }
  // FLAG.SPLAT_STATE: applies `op` with `bits` to the splats that pass (s & whereMask) == whereValue and for which
  // (hits >= minHits && maxWeight >= minWeight) == covered; covered = false names everything NOT seen.  Returns how many those are.
  stateCoverage({ minHits = 1, minWeight = 0, covered = true, whereMask = 0, whereValue = 0 } = {}, op, bits) {
    return loadNative().stateCoverage(this.handle, minHits >>> 0, +minWeight, covered ? 1 : 0, whereMask >>> 0, whereValue >>> 0, op >>> 0, bits >>> 0);
  }
  // Splat attributes: one f32 per resident splat, named by attr = {kind: ATTR.*, p: [..4]} -- p is the point of DIST2 (p[0..2]) or the
  // plane of PLANE (p . (x, y, z, 1); row 2 of the view matrix gives the depth) and ignored otherwise.  where = {mask, value} filters
  // like stateCount; the default is every splat, which needs no FLAG.SPLAT_STATE.  Every call completes the frames in flight first.
  // -> {matched, nan, min, max}: min / max over the values that are not NaN (-0 below +0), (Infinity, -Infinity) without any
  attrSummary(attr, { mask = 0, value = 0 } = {}) {
    return loadNative().attrSummary(this.handle, attr.kind >>> 0, attrParams(attr), mask >>> 0, value >>> 0);
  }
  // -> {counts: number[bins], below, above, nan}: v < lo below, v >= hi above, else bin min(trunc((v - lo) * f32(bins) / (hi - lo)), bins - 1)
  attrHistogram(attr, lo, hi, bins = 256, { mask = 0, value = 0 } = {}) {
    const c = new BigUint64Array(loadNative().attrHistogram(this.handle, attr.kind >>> 0, attrParams(attr), mask >>> 0, value >>> 0, +lo, +hi, bins >>> 0));
    const counts = Array.from(c.subarray(0, bins), Number);
    return { counts, below: Number(c[bins]), above: Number(c[bins + 1]), nan: Number(c[bins + 2]) };
  }
  // -> {values: Float32Array, ids: Uint32Array | null}: the matching splats' values in ascending index order (ids: their indices)
  attrValues(attr, { mask = 0, value = 0 } = {}, withIds = false) {
    const values = new Float32Array(loadNative().attrValues(this.handle, attr.kind >>> 0, attrParams(attr), mask >>> 0, value >>> 0));
    return { values, ids: withIds ? this.listState(mask, value) : null };
  }
  // FLAG.SPLAT_STATE: applies `op` with `bits` to the splats that pass (s & whereMask) == whereValue and for which
  // (lo <= v <= hi) == inside; a NaN is in no range, so {lo: -Infinity, hi: Infinity, inside: false} finds the broken splats.
  // Returns how many those are.
  stateAttr(attr, { lo = -Infinity, hi = Infinity, inside = true, whereMask = 0, whereValue = 0 } = {}, op, bits) {
    return loadNative().stateAttr(this.handle, attr.kind >>> 0, attrParams(attr), +lo, +hi, inside ? 1 : 0, whereMask >>> 0, whereValue >>> 0,
                                  op >>> 0, bits >>> 0);
  }
  // Neighbourhoods: for every splat that passes (qryMask, qryValue), how many splats that pass (srcMask, srcValue) lie within
  // `radius` of it (itself excluded, <= inclusive, the SPHERE region's f32 expression), saturated at `limit`, into a resident u32
  // plane; every other splat gets 0.  -> {queried, sources, candidates, cells, cellEdge}.  maxCandidates: the work budget (0: the
  // library's default); beyond it the call throws (code -8) and the plane stays.  Move or re-filter splats: count again.
  neighCount({ radius, limit = 0xFFFFFFFF, srcMask = 0, srcValue = 0, qryMask = 0, qryValue = 0, maxCandidates = 0 }) {
    return loadNative().neighCount(this.handle, +radius, limit >>> 0, srcMask >>> 0, srcValue >>> 0, qryMask >>> 0, qryValue >>> 0, +maxCandidates);
  }
  // -> Uint32Array: the count plane in splat order (zeros before the first neighCount and after an upload or a compaction)
  neighRead() { return new Uint32Array(loadNative().neighRead(this.handle)); }
  // FLAG.SPLAT_STATE: applies `op` with `bits` to the splats that pass (s & whereMask) == whereValue and whose count c has
  // (minCount <= c <= maxCount) == inside.  Returns how many those are.
  stateNeigh({ minCount = 0, maxCount = 0xFFFFFFFF, inside = true, whereMask = 0, whereValue = 0 } = {}, op, bits) {
    return loadNative().stateNeigh(this.handle, minCount >>> 0, maxCount >>> 0, inside ? 1 : 0, whereMask >>> 0, whereValue >>> 0, op >>> 0, bits >>> 0);
  }
  // Splat edits: bring splats back out of the library and make an edit permanent.  A splat matches when (s & mask) == value;
  // matching splats always come in ascending index order; (0, 0) is every splat and needs no FLAG.SPLAT_STATE.
  listState(mask, value) { return new Uint32Array(loadNative().listState(this.handle, mask >>> 0, value >>> 0)); }
  // -> {buffer: ArrayBuffer of 320-byte records (what PackedGaussians.fromRecords and an upload take), ids: their indices}
  exportSplats({ mask = 0, value = 0 } = {}) {
    const e = loadNative().exportSplats(this.handle, mask >>> 0, value >>> 0);
    return { buffer: e.records, ids: new Uint32Array(e.ids) };
  }
  // keeps the matching splats, drops the rest for good and renumbers; returns ids[new index] = old index (how a host renumbers
  // its own per-splat metadata).  State bytes are carried.  Like an upload: readPixels / readBuffer / pick need a new frame.
  compact(mask, value) {
    const ids = new Uint32Array(loadNative().compact(this.handle, mask >>> 0, value >>> 0));
    this.numGaussians = ids.length;
    return ids;
  }
  deleteHidden() { return this.compact(STATE.HIDDEN, 0); }
  // streams the matching splats into a binary 3DGS .ply (no whole-scene host buffer); returns how many were written
  savePly(file, { mask = 0, value = 0, shDegree = 3 } = {}) {
    return loadNative().exportPly(this.handle, String(file), mask >>> 0, value >>> 0, shDegree | 0);
  }
  // Splat transforms: applies what composeTransform returned, in place, to the resident splats with (s & mask) == value (default:
  // the selection; (0, 0): every splat); returns how many those are.  Not a frame and not an upload: the next frame sees the
  // moved splats.  The inverse transform is not a bit-exact undo: exportSplats first if one is needed.
  transformSplats(xform, mask = STATE.SELECTED, value = STATE.SELECTED) {
    return loadNative().transformSplats(this.handle, xform, mask >>> 0, value >>> 0);
  }
}

// composeTransform({rotation, translation, scale, pivot}) -> ArrayBuffer holding the gs_xform of p' = scale R (p - pivot) + pivot +
// translation, R the rotation of the quaternion `rotation` (r, x, y, z; any non-zero length).  Host mathematics (gs_xform_compose):
// no context, no GPU.  The buffer is opaque: hand it to renderer.transformSplats.
function composeTransform({ rotation = null, translation = null, scale = 1, pivot = null } = {}) {
  return loadNative().composeTransform(rotation, translation, scale, pivot);
}

// savePly(file, packedGaussians, shDegree): the inverse of PackedGaussians.fromFile (gs_ply_save; no context, no GPU)
function savePly(file, gaussians, shDegree = 3) {
  const buf = gaussians.gaussiansBuffer;
  const bytes = gaussians.numGaussians * 320;
  loadNative().savePly(String(file), bytes === buf.byteLength ? buf : buf.slice(0, bytes), shDegree | 0);
}

function attrParams(attr) {
  const p = new Float32Array(4);
  if (attr.p) p.set(Array.from(attr.p).slice(0, 4));
  return p;
}

const STATE = { HIDDEN: 0x1, SELECTED: 0x2, SET: 1, CLEAR: 2, TOGGLE: 3, ASSIGN: 4 };
const REGION = { ALL: 0, SPHERE: 1, BOX: 2, SCREEN_RECT: 3, SCREEN_MASK: 4 };

const COVERAGE = { REC_BYTES: 16 };
// byte offset of every field of a 16-byte gs_coverage_rec
const COVERAGE_FIELD = { sumQ: 0, hits: 8, maxWeight: 12 };

const PICK = { OK: 0, OUTSIDE_SLAB: 1, NONE: 0xFFFFFFFF, MAX_QUERIES: 65536, MAX_CONTRIB: 256 };
// word index of every field of a 48-byte gs_pick_result
const PICK_FIELD = { status: 0, listLength: 1, hitCount: 2, firstId: 3, firstDepth: 4, maxId: 5, maxWeight: 6, medianId: 7, medianDepth: 8,
                     alpha: 9, depthAcc: 10, reserved: 11 };
const PICK_F32 = new Set(['firstDepth', 'maxWeight', 'medianDepth', 'alpha', 'depthAcc']);
class PickResult {
  constructor(results, contrib, count, maxContrib) {
    this.count = count;
    this.maxContrib = maxContrib;
    this.bytes = results;                  // ArrayBuffer: count records of 48 bytes (gs_pick_result)
    this.u32 = new Uint32Array(results);   // word 12 q + PICK_FIELD.x for the integer fields
    this.f32 = new Float32Array(results);  // ... and for the float fields
    this.contribBytes = contrib;           // ArrayBuffer | null: count * maxContrib records {id u32, weight f32}
    this.contribId = contrib ? new Uint32Array(contrib) : null;      // word 2 (q maxContrib + k)
    this.contribWeight = contrib ? new Float32Array(contrib) : null; // word 2 (q maxContrib + k) + 1
  }
  get(q) {
    if (!(q >= 0 && q < this.count)) throw new RangeError('gsplat: pick result index out of range');
    const o = {};
    for (const [k, w] of Object.entries(PICK_FIELD)) o[k] = PICK_F32.has(k) ? this.f32[12 * q + w] : this.u32[12 * q + w];
    if (this.contribId) {
      o.contrib = [];
      for (let k = 0; k < this.maxContrib; ++k) {
        const i = 2 * (q * this.maxContrib + k);
        if (this.contribId[i] === PICK.NONE) break;
        o.contrib.push({ id: this.contribId[i], weight: this.contribWeight[i + 1] });
      }
    }
    return o;
  }
}

module.exports = { Renderer, loadNative, savePly, composeTransform, PickResult, PICK, PICK_FIELD, STATE, REGION, COVERAGE, COVERAGE_FIELD };
