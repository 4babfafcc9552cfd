'use strict';
// Driven by tests/test_napi_surface.py: node surface_check.js <command> <args...>; prints JSON on the last line of stdout.
// The N-API addon itself (loadNative()), not the Renderer class: what it exports, what it does with a wrong argument, and what
// its handle does with renderToSink frames in flight.
const fs = require('fs');
const path = require('path');
const g = require(path.join(__dirname, '..', '..', 'gaussian-splatting-wgpu_amd', 'js'));
const nat = g.loadNative();

const bytesOf = (file) => { const b = fs.readFileSync(file); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const same = (a, b) => { if (a.length !== b.length) return false; for (let i = 0; i < a.length; ++i) if (a[i] !== b[i]) return false; return true; };
// [class name, message, code] of what fn() throws; null if it returns
function thrown(fn) {
  try { fn(); return null; } catch (e) { return [e.constructor.name, e.message, e.code === undefined ? null : e.code]; }
}

// Every export that takes a context handle first, with arguments of the right types (U: a uniform block, S: a sink).
function contextCalls(U, S) {
  const p = new Float32Array(4), ids = new Uint32Array(2), xf = nat.composeTransform(null, null, null, null);
  return {
    uploadSplats: [new ArrayBuffer(320), 1], shareSplats: [{}], renderSync: [U], renderAsync: [U], readRgba8: [], readBuffer: [8],
    pick: [new Uint32Array(2), 0], accumulateCoverage: [null], resetCoverage: [], readCoverage: [], stateCoverage: [1, 0, 1, 0, 0, 1, 2],
    attrSummary: [0, p, 0, 0], attrHistogram: [0, p, 0, 0, 0, 1, 8], attrValues: [0, p, 0, 0], stateAttr: [0, p, 0, 1, 1, 0, 0, 1, 2],
    neighCount: [0.5, 7, 0, 0, 0, 0, 0], neighRead: [], stateNeigh: [0, 2, 1, 0, 0, 1, 2], stateRegion: [{ kind: 0 }, 1, 2], stateIds: [ids, 1, 2],
    stateCount: [0, 0], readState: [], writeState: [new Uint8Array(4)], setOption: [11, 0], listState: [0, 0], exportSplats: [0, 0], compact: [0, 0],
    exportPly: ['/nonexistent/x.ply', 0, 0, 3], transformSplats: [xf, 0, 0], stats: [], slab: [], uploadPly: ['/nonexistent/x.ply'],
    renderToSink: [U, S],
  };
}

async function main() {
  const cmd = process.argv[2];
  if (cmd === 'surface') {
    const functions = [], constants = {};
    for (const k of Object.keys(nat)) { if (typeof nat[k] === 'function') functions.push(k); else constants[k] = nat[k]; }
    console.log(JSON.stringify({ functions, constants }));
  } else if (cmd === 'nocontext') {
    // nocontext <records.bin (3 x 320 B)> <out.ply> <out records.bin>
    const out = {};
    out.createEmpty = thrown(() => nat.create({}));
    const x = nat.composeTransform(null, null, null, null);
    out.xform = Array.from(new Uint8Array(x));
    out.zeroQuat = thrown(() => nat.composeTransform([0, 0, 0, 0], null, null, null));
    const rec = bytesOf(process.argv[3]);
    out.saved = nat.savePly(process.argv[4], rec, 3) === undefined;
    const l = nat.loadPly(process.argv[4]);
    out.loaded = { n: l.n, degree: l.degree, keys: Object.keys(l).sort(), bytes: l.records.byteLength };
    fs.writeFileSync(process.argv[5], Buffer.from(l.records));
    out.hostAlloc0 = thrown(() => nat.hostAlloc(0));
    console.log(JSON.stringify(out));
  } else if (cmd === 'nodevice') {
    console.log(JSON.stringify({ create: thrown(() => nat.create({ width: 64, height: 64 })) }));
  } else if (cmd === 'nohandle') {
    // every context-taking export with {} for the handle; destroy({}) returns undefined
    const calls = contextCalls(new Float32Array(40), new Uint8Array(16));
    const out = { destroy: nat.destroy({}) === undefined, calls: {} };
    for (const name of Object.keys(calls)) out.calls[name] = thrown(() => nat[name]({}, ...calls[name]));
    console.log(JSON.stringify(out));
  } else if (cmd === 'misuse') {
    // misuse <records.bin> <n> <W> <H> <uniforms.bin>: on a live handle, every context-taking export once per argument position
    // with a wrong-typed or too-short value: [export, position, what replaces the good argument].  Only what the addon refuses
    // before anything is launched; the expectations are in test_napi_surface.py.
    const n = parseInt(process.argv[4], 10), W = parseInt(process.argv[5], 10), H = parseInt(process.argv[6], 10);
    const U = new Float32Array(bytesOf(process.argv[7]));
    const h = nat.create({ width: W, height: H, tileSize: 16, device: 0, flags: nat.FLAG_SPLAT_STATE });
    nat.uploadSplats(h, bytesOf(process.argv[3]), n);
    const O = {}, B3 = new Uint8Array(3), STR = 'text';
    const each = (fn, positions, bad) => positions.map((k) => [fn, k, bad]);
    const table = [
      ['uploadSplats', 1, STR], ['uploadSplats', 1, B3], ['uploadSplats', 2, O], ['uploadSplats', 2, -1], ['uploadSplats', 2, 0.5],
      ['shareSplats', 1, O], ['renderSync', 1, B3], ['renderSync', 1, STR], ['renderAsync', 1, B3], ['renderAsync', 1, STR], ['readBuffer', 1, O],
      ['pick', 1, STR], ['pick', 1, B3], ['pick', 1, new Uint32Array(0)], ['pick', 2, O], ['pick', 2, 257],
      ['accumulateCoverage', 1, { x0: 0 }], ['accumulateCoverage', 1, { x0: 0, y0: 0, x1: 1, y1: 1, mask: new Uint8Array(4) }],
      ['accumulateCoverage', 1, { x0: 0, y0: 0, x1: 1, y1: 1, mask: B3, maskWidth: 4, maskHeight: 4 }],
      ...each('stateCoverage', [1, 2, 3, 4, 5, 6, 7], O),
      ['attrSummary', 1, O], ['attrSummary', 2, new Float32Array(3)], ['attrSummary', 2, STR], ...each('attrSummary', [3, 4], O),
      ['attrHistogram', 1, O], ['attrHistogram', 2, new Float32Array(3)], ...each('attrHistogram', [3, 4, 5, 6, 7], O),
      ['attrValues', 1, O], ['attrValues', 2, new Float32Array(3)], ...each('attrValues', [3, 4], O),
      ['stateAttr', 1, O], ['stateAttr', 2, new Float32Array(3)], ...each('stateAttr', [3, 4, 5, 6, 7, 8, 9], O),
      ...each('neighCount', [1, 2, 3, 4, 5, 6, 7], O), ...each('stateNeigh', [1, 2, 3, 4, 5, 6, 7], O),
      ['stateRegion', 1, O], ['stateRegion', 1, 5], ['stateRegion', 1, { kind: 0, uniforms: B3 }], ['stateRegion', 1, { kind: 0, mask: B3 }],
      ...each('stateRegion', [2, 3], O),
      ['stateIds', 1, STR], ['stateIds', 1, B3], ...each('stateIds', [2, 3], O), ...each('stateCount', [1, 2], O), ['writeState', 1, STR],
      ...each('setOption', [1, 2], O), ...each('listState', [1, 2], O), ...each('exportSplats', [1, 2], O), ...each('compact', [1, 2], O),
      ...each('exportPly', [1, 2, 3, 4], O), ['transformSplats', 1, B3], ['transformSplats', 1, STR], ...each('transformSplats', [2, 3], O),
      ['uploadPly', 1, O], ['renderToSink', 1, B3], ['renderToSink', 2, STR],
    ];
    const good = contextCalls(U, new Uint8Array(W * H * 4));
    const rows = [];
    for (const [fn, k, bad] of table) {
      const args = good[fn].slice();
      args[k - 1] = bad;
      const label = typeof bad === 'object' ? (ArrayBuffer.isView(bad) ? bad.constructor.name + '(' + bad.length + ')' : JSON.stringify(Object.keys(bad))) : JSON.stringify(bad);
      rows.push({ fn, pos: k, bad: label, got: thrown(() => nat[fn](h, ...args)) });
    }
    const framesAfter = nat.stats(h).frames;
    nat.renderSync(h, U);
    const bytes = nat.readRgba8(h).byteLength;
    nat.destroy(h);
    console.log(JSON.stringify({ rows, exports: Object.keys(good), framesAfter, bytes }));
  } else if (cmd === 'sinkflight') {
    // sinkflight <records.bin> <n> <W> <H> <uniforms.bin (3 x 160 B)>: three renderToSink frames outstanding on one handle
    const n = parseInt(process.argv[4], 10), W = parseInt(process.argv[5], 10), H = parseInt(process.argv[6], 10);
    const ub = bytesOf(process.argv[7]);
    const us = [0, 1, 2].map((k) => new Float32Array(ub.slice(160 * k, 160 * (k + 1))));
    const b = nat.create({ width: W, height: H, tileSize: 16, device: 0 }); // owns the splats and outlives h
    nat.uploadSplats(b, bytesOf(process.argv[3]), n);
    const h = nat.create({ width: W, height: H, tileSize: 16, device: 0 });
    nat.shareSplats(h, b);
    const want = us.map((u) => { nat.renderSync(b, u); return new Uint8Array(nat.readRgba8(b)); });
    const sinks = us.map(() => new Uint8Array(nat.hostAlloc(W * H * 4)));
    const ps = us.map((u, k) => nat.renderToSink(h, u, sinks[k]));
    const out = {};
    out.renderAsync = thrown(() => nat.renderAsync(h, us[0]));
    out.stats = thrown(() => nat.stats(h));
    out.destroy = nat.destroy(h) === undefined; // deferred: three workers are waiting on the context's tickets
    out.resolved = (await Promise.all(ps)).map((v) => v === undefined);
    out.same = sinks.map((s, k) => same(s, want[k]));
    out.bytes = sinks.map((s) => s.length);
    out.after = thrown(() => nat.stats(h));
    nat.destroy(b);
    console.log(JSON.stringify(out));
  } else {
    throw new Error('unknown command ' + cmd);
  }
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
