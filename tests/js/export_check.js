'use strict';
// Driven by tests/test_export.py: node export_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <hide.bin> <out.bin> <a.ply> <b.ply>
// Hides the given splats, lists the rest, deletes the hidden ones, renders, exports and saves through the Node host; writes the
// listed ids, the id map, the frame, the exported records and their ids to <out.bin>, the streamed file to <a.ply> and the
// module-level savePly of the exported buffer to <b.ply>.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const rec = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10), W = parseInt(process.argv[4], 10), H = parseInt(process.argv[5], 10), ts = parseInt(process.argv[6], 10);
const ub = fs.readFileSync(process.argv[7]);
const hb = fs.readFileSync(process.argv[8]);
const u = new Float32Array(ub.buffer.slice(ub.byteOffset, ub.byteOffset + 160));
const hide = new Uint32Array(hb.buffer.slice(hb.byteOffset, hb.byteOffset + hb.byteLength));
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const cam = { packUniforms: (w, h, out) => { out.set(u); return out; } };
const ic = { isDirty() { return false; }, getCamera() { return cam; } }; // frames are rendered explicitly below
const { STATE } = g;
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
r.stateIds(hide, STATE.SET, STATE.HIDDEN);
const listed = r.listState(STATE.HIDDEN, 0);
const ids = r.deleteHidden();
r.renderUniforms(u);
const img = r.readPixels();
const ex = r.exportSplats();
const saved = r.savePly(process.argv[10]);
g.savePly(process.argv[11], g.PackedGaussians.fromRecords(ex.buffer, ex.ids.length), 3); // the exported buffer is a PackedGaussians buffer
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
fs.writeFileSync(process.argv[9], Buffer.concat([bytes(listed), bytes(ids), Buffer.from(img), Buffer.from(ex.buffer), bytes(ex.ids)]));
const errors = {};
try { r.listState(0x100, 0); errors.badMask = 'none'; } catch (e) { errors.badMask = e.code; }
const plain = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: 0, shareWith: r }, pg, ts);
try { plain.compact(STATE.HIDDEN, 0); errors.unflagged = 'none'; } catch (e) { errors.unflagged = e.code; }
plain.destroy().then(() => r.destroy()).then(() => console.log(JSON.stringify({ kept: ids.length, listed: listed.length, numGaussians: r.numGaussians, saved, errors })));
