'use strict';
// Driven by tests/test_coverage.py: node coverage_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <x0> <y0> <x1> <y1> <mask.bin> <out.bin>
// Renders one frame on the product path, accumulates the rect AND the mask twice over (reset in between is checked), applies
// stateCoverage and writes the plane bytes followed by the state bytes.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const a = process.argv;
const rec = fs.readFileSync(a[2]);
const n = parseInt(a[3], 10), W = parseInt(a[4], 10), H = parseInt(a[5], 10), ts = parseInt(a[6], 10);
const ub = fs.readFileSync(a[7]);
const [x0, y0, x1, y1] = [a[8], a[9], a[10], a[11]].map((v) => parseInt(v, 10));
const mb = fs.readFileSync(a[12]);
const u = new Float32Array(ub.buffer.slice(ub.byteOffset, ub.byteOffset + 160));
const mask = new Uint8Array(mb.buffer.slice(mb.byteOffset, mb.byteOffset + mb.byteLength));
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const cam = { packUniforms: (w, h, out) => { out.set(u); return out; } };
const ic = { isDirty() { return false; }, getCamera() { return cam; } }; // frames are rendered explicitly below
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
const zeroBefore = new Uint32Array(r.readCoverage().bytes).every((v) => v === 0);
r.renderUniforms(u);
const whole = r.accumulateCoverage();
r.resetCoverage();
const zeroAfterReset = new Uint32Array(r.readCoverage().bytes).every((v) => v === 0);
const pixels = r.accumulateCoverage({ x0, y0, x1, y1, mask });
const cov = r.readCoverage();
const matched = r.stateCoverage({ minHits: 2, minWeight: 0.05, covered: true }, g.STATE.SET, g.STATE.SELECTED);
const unseen = r.stateCoverage({ covered: false }, g.STATE.SET, g.STATE.HIDDEN);
fs.writeFileSync(a[13], Buffer.concat([Buffer.from(cov.bytes), Buffer.from(r.readState())]));
let best = 0;
for (let i = 1; i < cov.count; ++i) if (cov.u32[4 * i + g.COVERAGE_FIELD.hits / 4] > cov.u32[4 * best + g.COVERAGE_FIELD.hits / 4]) best = i;
const errors = {};
try { r.accumulateCoverage({ x0: 0, y0: 0, x1: W + 1, y1: H }); errors.outside = 'none'; } catch (e) { errors.outside = e.code; }
try { r.accumulateCoverage({ x0: 5, y0: 0, x1: 5, y1: H }); errors.empty = 'none'; } catch (e) { errors.empty = e.code; }
r.destroy().then(() => console.log(JSON.stringify({
  n: cov.count, whole, pixels, matched, unseen, zeroBefore, zeroAfterReset, errors,
  most_hits: { id: best, hits: cov.u32[4 * best + g.COVERAGE_FIELD.hits / 4], sumQ: cov.u64[2 * best + g.COVERAGE_FIELD.sumQ / 8].toString(),
               maxWeight: cov.f32[4 * best + g.COVERAGE_FIELD.maxWeight / 4] } })));
