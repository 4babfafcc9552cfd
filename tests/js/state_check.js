'use strict';
// Driven by tests/test_splat_state.py: node state_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <mask.bin> <ids.bin> <out.bin>
// Runs a short sequence of state calls through the Node host, renders, and writes the state plane, the frame, and the frame after
// writeState(zeros).
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const rec = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10), W = parseInt(process.argv[4], 10), H = parseInt(process.argv[5], 10), ts = parseInt(process.argv[6], 10);
const ub = fs.readFileSync(process.argv[7]);
const mb = fs.readFileSync(process.argv[8]);
const ib = fs.readFileSync(process.argv[9]);
const u = new Float32Array(ub.buffer.slice(ub.byteOffset, ub.byteOffset + 160));
const mask = new Uint8Array(mb.buffer.slice(mb.byteOffset, mb.byteOffset + mb.byteLength));
const ids = new Uint32Array(ib.buffer.slice(ib.byteOffset, ib.byteOffset + ib.byteLength));
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const cam = { packUniforms: (w, h, out) => { out.set(u); return out; } };
const ic = { isDirty() { return false; }, getCamera() { return cam; } }; // frames are rendered explicitly below
const { STATE, REGION } = g;
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
const matched = [
  r.stateRegion({ kind: REGION.SCREEN_RECT, x0: W >> 2, y0: H >> 2, x1: (3 * W) >> 2, y1: (3 * H) >> 2, uniforms: u }, STATE.SET, STATE.SELECTED),
  r.stateRegion({ kind: REGION.SCREEN_MASK, mask, uniforms: u, whereMask: STATE.SELECTED, whereValue: 0 }, STATE.SET, 0x10),
  r.stateRegion({ kind: REGION.SPHERE, a: [0.5, 0.2, -0.3], b: [0.75, 0, 0] }, STATE.SET, STATE.HIDDEN),
  r.stateRegion({ kind: REGION.BOX, a: [-1.0, -0.5, -1.0], b: [0.5, 1.0, 1.5] }, STATE.TOGGLE, 0x20),
];
r.stateIds(ids, STATE.TOGGLE, 0x40);
r.setOption(g.OPT.SELECT_TINT, 0xC03380E6);
const plane = r.readState();
r.renderUniforms(u);
const img = r.readPixels();
const counts = [r.stateCount(STATE.HIDDEN, STATE.HIDDEN), r.stateCount(0xFF, 0)];
r.writeState(new Uint8Array(n));
r.renderUniforms(u);
const img0 = r.readPixels();
fs.writeFileSync(process.argv[10], Buffer.concat([Buffer.from(plane), Buffer.from(img), Buffer.from(img0)]));
const errors = {};
try { r.stateIds(new Uint32Array([1, n]), STATE.SET, 1); errors.badId = 'none'; } catch (e) { errors.badId = e.code; }
try { r.stateIds([1, 2], STATE.SET, 1); errors.notTyped = 'none'; } catch (e) { errors.notTyped = e.name; }
const plain = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: 0, shareWith: r }, pg, ts);
try { plain.stateCount(0, 0); errors.unflagged = 'none'; } catch (e) { errors.unflagged = e.code; }
plain.destroy().then(() => r.destroy()).then(() => console.log(JSON.stringify({ matched, counts, errors })));
