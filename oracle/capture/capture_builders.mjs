// Runs the reference's own BVH builders (lib/BVH/bvhNode.js: generate_bvh_heirarchy and generate_bvh_heirarchy_SAH, through
// lib/BVH/bvhBuilder.js's populate_links / flattenBVH, imported unchanged from /root/reference) on the in-domain box sets of
// tests/builder_cases.py and records what they make:
//     python tests/builder_cases.py                  (writes tests/golden/builder/cases.json and boxes_*.f64.gz)
//     cd oracle/capture && node --experimental-loader ./loader.mjs capture_builders.mjs
// Outputs are DATA only: tests/golden/builder/reference.json (rows and sha256 per case and builder) and reference_rows.bin.gz (the rows as
// Float32Array bytes and the order as Int32Array bytes, for the cases of at most `stored_max` primitives).  Boxes outside the builders'
// domain are never fed to the reference: its SAH loop only ends at its 500,000-entry stack limit on them.
import fs from 'fs';
import path from 'path';
import zlib from 'zlib';
import crypto from 'crypto';
import { performance } from 'perf_hooks';

const REF = '/root/reference/';
const DIR = path.resolve(path.dirname(new URL(import.meta.url).pathname), '../../tests/golden/builder');
globalThis.performance = performance;
const say = console.log; console.log = () => {};

const sha = (ta) => crypto.createHash('sha256').update(Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)).digest('hex');

async function main() {
  const { AABB } = await import('file://' + REF + 'lib/BVH/AABB.js');
  const { BVH } = await import('file://' + REF + 'lib/BVH/bvhNode.js');
  const { build_bvh } = await import('file://' + REF + 'lib/BVH/bvhBuilder.js');
  const median = BVH.create_bvh;
  const sah = (objs) => ({ bvh: BVH.generate_bvh_heirarchy_SAH(objs, 0, objs.length - 1), objs: objs });  // as capture.mjs routes it

  const man = JSON.parse(fs.readFileSync(path.join(DIR, 'cases.json'), 'utf8'));
  const files = {};
  const doubles = (file) => {
    if (!files[file]) {
      const raw = zlib.gunzipSync(fs.readFileSync(path.join(DIR, file)));
      files[file] = new Float64Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
    }
    return files[file];
  };
  const out = {}, chunks = [];
  let at = 0;
  const keep = (ta) => { const b = Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength); chunks.push(b); at += b.length; return at - b.length; };
  for (const c of man.cases) {
    const set = man.sets.find((s) => s.family === c.family && s.n === c.n);
    const d = doubles(set.file), n = c.n;
    const rec = { n: n };
    for (const [tag, create] of [['median', median], ['sah', sah]]) {
      const objs = [];
      for (let i = 0; i < n; i++) {
        const box = new AABB();
        box.min = [0, 1, 2].map((k) => d[set.offset + 3 * i + k] * c.scale);
        box.max = [0, 1, 2].map((k) => d[set.offset + 3 * n + 3 * i + k] * c.scale);
        objs.push({ bbox: box, type: 2, input: i });
      }
      BVH.create_bvh = create;
      const built = build_bvh(objs);
      const rows = new Float32Array(built.flattened_array.flat());   // lib/scene.js:304
      const order = new Int32Array(built.bvh.objs.map((o) => o.input));
      const e = { n_rows: rows.length / 12, rows_sha256: sha(rows), order_sha256: sha(order), stored: n <= man.stored_max };
      if (e.stored) { e.rows_at = keep(rows); e.order_at = keep(order); }
      rec[tag] = e;
    }
    out[c.name] = rec;
  }
  BVH.create_bvh = median;
  fs.writeFileSync(path.join(DIR, 'reference_rows.bin.gz'), zlib.gzipSync(Buffer.concat(chunks), { level: 9 }));
  fs.writeFileSync(path.join(DIR, 'reference.json'), JSON.stringify(out, null, 1));
  console.log = say;
  console.log('wrote', Object.keys(out).length, 'cases to', DIR);
}
main().catch((e) => { console.error(e); process.exit(1); });
