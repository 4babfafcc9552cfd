'use strict';
// Driven by tests/test_pick.py: node pick_check.js <records.bin> <n> <W> <H> <tile> <uniforms.bin> <queries.bin> <maxContrib> <out.bin>
// Renders one frame on the product path, picks the queries (u32 x,y pairs) and writes the result bytes followed by the contributor bytes.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const rec = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10), W = parseInt(process.argv[4], 10), H = parseInt(process.argv[5], 10), ts = parseInt(process.argv[6], 10);
const ub = fs.readFileSync(process.argv[7]);
const qb = fs.readFileSync(process.argv[8]);
const maxContrib = parseInt(process.argv[9], 10);
const u = new Float32Array(ub.buffer.slice(ub.byteOffset, ub.byteOffset + 160));
const queries = new Uint32Array(qb.buffer.slice(qb.byteOffset, qb.byteOffset + qb.byteLength));
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const cam = { packUniforms: (w, h, out) => { out.set(u); return out; } };
const ic = { isDirty() { return false; }, getCamera() { return cam; } }; // frames are rendered explicitly below
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: 0 }, pg, ts);
r.renderUniforms(u);
const p = r.pick(queries, maxContrib);
fs.writeFileSync(process.argv[10], Buffer.concat([Buffer.from(p.bytes), Buffer.from(p.contribBytes)]));
let best = 0;
for (let q = 1; q < p.count; ++q) if (p.u32[12 * q + g.PICK_FIELD.hitCount] > p.u32[12 * best + g.PICK_FIELD.hitCount]) best = q;
const errors = {};
try { r.pick(new Uint32Array([W, 0])); errors.outside = 'none'; } catch (e) { errors.outside = e.code; }
try { r.pick(new Uint32Array([1, 2, 3])); errors.odd = 'none'; } catch (e) { errors.odd = e.name; }
r.destroy().then(() => console.log(JSON.stringify({ n: p.count, most_hits: Object.assign({ q: best }, p.get(best)), errors })));
