'use strict';
// Driven by tests/test_aux_planes.py: node aux_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <out.bin>
// Renders one EXACT frame with FLAG.AUX_OUTPUTS and writes readAlpha(), readDepth() and readDepth(true) (f32 planes, in that order).
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
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.EXACT_BLEND | g.FLAG.AUX_OUTPUTS }, pg, ts);
r.renderUniforms(u);
const a = r.readAlpha(), d = r.readDepth(), dn = r.readDepth(true);
const out = Buffer.concat([Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(d.buffer, d.byteOffset, d.byteLength),
                           Buffer.from(dn.buffer, dn.byteOffset, dn.byteLength)]);
fs.writeFileSync(process.argv[8], out);
r.destroy().then(() => console.log(JSON.stringify({ n: a.length })));
