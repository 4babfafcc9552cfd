'use strict';
// Driven by tests/test_attributes.py: node attr_check.js <records.bin> <n> <W> <H> <tile>
// Marks the splats within 1.5 of the origin with host bit 0x04, then prints the opacity logit's summary, 16-bin histogram over
// [-2, 3) and first values, dense and for the marked splats, the largest DIST2, and what stateAttr matched.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const a = process.argv;
const rec = fs.readFileSync(a[2]);
const n = parseInt(a[3], 10), W = parseInt(a[4], 10), H = parseInt(a[5], 10), ts = parseInt(a[6], 10);
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const ic = { isDirty() { return false; }, getCamera() { return null; } }; // no frame is rendered
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
r.stateRegion({ kind: g.REGION.SPHERE, a: [0, 0, 0], b: [1.5, 0, 0] }, g.STATE.SET, 0x04);
const logit = { kind: g.ATTR.OPACITY_LOGIT };
const answer = (where) => {
  const s = r.attrSummary(logit, where);
  const v = r.attrValues(logit, where, true);
  return { matched: s.matched, nan: s.nan, min: s.min, max: s.max, histogram: r.attrHistogram(logit, -2, 3, 16, where), count: v.values.length,
           first: Array.from(v.values.subarray(0, 8)), firstIds: Array.from(v.ids.subarray(0, 8)) };
};
const dense = answer(undefined), filtered = answer({ mask: 0x04, value: 0x04 });
const dist2Max = r.attrSummary({ kind: g.ATTR.DIST2, p: [0.5, 0.2, -0.3] }).max;
const stateAttr = r.stateAttr(logit, { hi: 0, whereMask: 0x04, whereValue: 0x04 }, g.STATE.SET, g.STATE.SELECTED);
const selected = r.stateCount(g.STATE.SELECTED, g.STATE.SELECTED);
const nanFinder = r.stateAttr(logit, { inside: false }, g.STATE.SET, 0x40);
const errors = {};
try { r.attrSummary({ kind: 16 }); errors.kind = 'none'; } catch (e) { errors.kind = e.code; }
try { r.attrHistogram(logit, 0, 1, 1025); errors.bins = 'none'; } catch (e) { errors.bins = e.code; }
r.destroy().then(() => console.log(JSON.stringify({ dense, filtered, dist2Max, stateAttr, selected, nanFinder, errors })));
