'use strict';
// Driven by tests/test_neighbours.py: node neigh_check.js <records.bin> <n> <W> <H> <tile>
// Counts the neighbours within 0.5 (limit 7), prints the info, the plane's length, sum, first counts and histogram, what stateNeigh
// matched for counts 0 .. 2; then marks the splats within 1.5 of the origin with host bit 0x04 and counts, for the unmarked ones,
// whether a marked one lies within 0.5; and the codes of three refused calls.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));

const a = process.argv;
const rec = fs.readFileSync(a[2]);
const n = parseInt(a[3], 10), W = parseInt(a[4], 10), H = parseInt(a[5], 10), ts = parseInt(a[6], 10);
const pg = g.PackedGaussians.fromRecords(rec.buffer.slice(rec.byteOffset, rec.byteOffset + rec.byteLength), n);
const ic = { isDirty() { return false; }, getCamera() { return null; } }; // no frame is rendered
const r = new g.Renderer({ width: W, height: H, manual: true }, ic, { ordinal: 0, flags: g.FLAG.SPLAT_STATE }, pg, ts);
const info = r.neighCount({ radius: 0.5, limit: 7 });
const c = r.neighRead();
const histogram = new Array(8).fill(0);
let sum = 0;
for (const v of c) { histogram[v] += 1; sum += v; }
const stateNeigh = r.stateNeigh({ minCount: 0, maxCount: 2 }, g.STATE.SET, g.STATE.SELECTED);
const selected = r.stateCount(g.STATE.SELECTED, g.STATE.SELECTED);
r.stateRegion({ kind: g.REGION.SPHERE, a: [0, 0, 0], b: [1.5, 0, 0] }, g.STATE.SET, 0x04);
r.neighCount({ radius: 0.5, limit: 1, srcMask: 4, srcValue: 4, qryMask: 4, qryValue: 0 });
let filteredSum = 0;
for (const v of r.neighRead()) filteredSum += v;
const errors = {};
try { r.neighCount({ radius: -1 }); errors.radius = 'none'; } catch (e) { errors.radius = e.code; }
try { r.neighCount({ radius: 0.5, limit: 0 }); errors.limit = 'none'; } catch (e) { errors.limit = e.code; }
try { r.neighCount({ radius: 0.5, maxCandidates: 1 }); errors.budget = 'none'; } catch (e) { errors.budget = e.code; }
r.destroy().then(() => console.log(JSON.stringify({ info, length: c.length, sum, first: Array.from(c.subarray(0, 16)), histogram, stateNeigh, selected,
                                                    filteredSum, errors })));
