'use strict';
// Driven by tests/test_transform.py: node xform_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <out.bin>
// Selects the unit sphere, composes a similarity and applies it to the selection through the Node host, renders and exports; writes
// the composed struct, the frame and the exported records to <out.bin>.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const rec = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10), W = parseInt(process.argv[4], 10), H = parseInt(process.argv[5], 10), ts = parseInt(process.argv[6], 10);
const ub = fs.readFileSync(process.argv[7]);
const u = new Float32Array(ub.buffer.slice(ub.byteOffset, ub.byteOffset + 160));
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const cam = { packUniforms: (w, h, out) => { out.set(u); return out; } };
const ic = { isDirty() { return false; }, getCamera() { return cam; } }; // frames are rendered explicitly below
const { STATE, REGION } = g;
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
const selected = r.stateRegion({ kind: REGION.SPHERE, a: [0, 0, 0], b: [1, 0, 0] }, STATE.SET, STATE.SELECTED);
const x = g.composeTransform({ rotation: [0.9, 0.1, -0.3, 0.2], translation: [0.15, 0.1, -0.2], scale: 1.3, pivot: [0.1, 0.0, -0.1] });
const matched = r.transformSplats(x);
r.renderUniforms(u);
const img = r.readPixels();
const ex = r.exportSplats();
fs.writeFileSync(process.argv[8], Buffer.concat([Buffer.from(x), Buffer.from(img), Buffer.from(ex.buffer)]));
const noop = new Uint8Array(g.composeTransform()); // the identity: POSITION only
const flagsOf = (b) => new Uint32Array(b.slice(0, 8))[1];
new Uint32Array(noop.buffer)[1] = 0; // flags = 0: a valid no-op that still counts
const matchedAll = r.transformSplats(noop.buffer, 0, 0);
const errors = {};
try { r.transformSplats(x, 0x100, 0); errors.badMask = 'none'; } catch (e) { errors.badMask = e.code; }
try { g.composeTransform({ rotation: [0, 0, 0, 0] }); errors.zeroQuaternion = 'none'; } catch (e) { errors.zeroQuaternion = e.code; }
const b = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE, shareWith: r }, pg, ts);
try { b.transformSplats(x); errors.borrower = 'none'; } catch (e) { errors.borrower = e.code; }
b.destroy().then(() => r.destroy()).then(() => console.log(JSON.stringify({ selected, matched, matchedAll, structBytes: x.byteLength, flags: flagsOf(x), errors })));
