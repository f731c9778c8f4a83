// Captures the `edge_geometry` scene of tests/edge_geometry.py from the reference's own Scene (lib/scene.js and friends, imported unchanged from
// /root/reference), as capture.mjs captures c2m: a Cornell box and tests/golden/assets/edge_geometry.obj.gz three times over under three transforms.
//     python tests/edge_geometry.py                  (writes the OBJ fixture)
//     cd oracle/capture && node --experimental-loader ./loader.mjs capture_edge.mjs
// Outputs are DATA only: tests/golden/edge_*.bin (the seven buffers with the median tree), edgesah_bvh.bin / edgesah_triangles.bin (the same scene
// through BVH.generate_bvh_heirarchy_SAH) and edge_manifest.json.
import fs from 'fs';
import path from 'path';
import zlib from 'zlib';
import crypto from 'crypto';
import { performance } from 'perf_hooks';

const REF = '/root/reference/';
const OUT = path.resolve(path.dirname(new URL(import.meta.url).pathname), '../../tests/golden');
globalThis.performance = performance;
globalThis.fetch = async (p) => ({ text: async () => zlib.gunzipSync(fs.readFileSync(path.join(OUT, 'assets', path.basename(p) + '.gz'))).toString('utf8') });
const say = console.log; console.log = () => {};

const sha = (ta) => crypto.createHash('sha256').update(Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)).digest('hex');
const manifest = {};
function save(scene, name, ta) {
  manifest[scene] = manifest[scene] || {};
  manifest[scene][name] = { dtype: ta instanceof Int32Array ? 'i32' : 'f32', length: ta.length, sha256: sha(ta) };
  fs.writeFileSync(path.join(OUT, `${scene}_${name}.bin`), Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength));
}

async function main() {
  const { Scene } = await import('file://' + REF + 'lib/scene.js');
  const { Quad } = await import('file://' + REF + 'lib/primitives/quad.js');
  const { Mesh } = await import('file://' + REF + 'lib/primitives/mesh.js');
  const { ObjReader } = await import('file://' + REF + 'lib/primitives/objReader.js');
  const { BVH } = await import('file://' + REF + 'lib/BVH/bvhNode.js');
  const { mat4 } = await import('../../webgpu-path-tracer_amd/js/glmatrix.mjs');

  Scene.prototype.create_spheres = function () {
    this.add_material('default', 0, [1, 0, 0], [0, 0, 0], [0, 0, 0], 0, 0, 0);
    this.objs.push(this.spheres.flat());
  };
  Scene.prototype.create_quads = function () {   // the Cornell box of capture.mjs
    this.add_material('red', 0, [0.75, 0.1, 0.1], [0.75, 0.1, 0.1], [0, 0, 0], 0.05, 0.95, 0);
    this.add_material('green', 0, [0.05, 0.55, 0.05], [0.05, 0.55, 0.05], [0, 0, 0], 0.05, 0.95, 0);
    this.add_material('blue', 0, [0.05, 0.05, 0.55], [0.05, 0.05, 0.55], [0, 0, 0], 0.05, 0.95, 0);
    this.add_material('white', 0, [0.76, 0.70, 0.51], [0.76, 0.70, 0.51], [0, 0, 0], 0.05, 0.95, 0);
    this.add_material('glossywhite', 0, [0.76, 0.70, 0.51], [0.76, 0.70, 0.51], [0, 0, 0], 0.3, 0.1, 0);
    this.add_material('black', 0, [0.2, 0.2, 0.2], [0.2, 0.2, 0.2], [0, 0, 0], 0.05, 0.95, 0);
    this.add_material('glass', 1, [0.95, 0.95, 0.95], [0, 0, 0], [0, 0, 0], 0, 0, 0);
    this.quads.push(
      new Quad([-0.35, 0.9999, -0.3], [0.7, 0, 0], [0, 0, 0.6], this.global_id++, this.quad_id++, this.add_material('light', 0, [0, 0, 0], [0, 0, 0], [10, 10, 10], 0, 0, 0)),
      new Quad([-1, -1, -1], [2, 0, 0], [0, 2, 0], this.global_id++, this.quad_id++, this.material_dict['black']),
      new Quad([-1, -1, 1], [0, 0, -2], [0, 2, 0], this.global_id++, this.quad_id++, this.material_dict['red']),
      new Quad([1, -1, -1], [0, 0, 2], [0, 2, 0], this.global_id++, this.quad_id++, this.material_dict['green']),
      new Quad([-1, 1, -1], [2, 0, 0], [0, 0, 2], this.global_id++, this.quad_id++, this.material_dict['white']),
      new Quad([1, -1, -1], [-2, 0, 0], [0, 0, 2], this.global_id++, this.quad_id++, this.material_dict['glossywhite']),
    );
    this.lights.push(this.quads[0]);
    this.objs.push(this.quads.flat());
  };
  Scene.prototype.init_mesh_data = async function () { this.mesh_data = { edge: await ObjReader.load_model('./assets/edge_geometry.obj') }; };
  Scene.prototype.create_meshes = function () {
    const poses = [
      (t) => t.update(t.scale(0.25, 1, 1)),
      (t) => t.update(t.scale(0.3, 0.2, 0.4), t.rotate(0.7, [0.3, 1.0, 0.2]), t.translate(0.1, -0.3, 0.1)),
      (t) => {
        t.update(t.scale(0.5, 0.5, 0.5), t.translate(0, 0, -0.2));
        t.modelMatrix[3] = 1; t.modelMatrix[7] = 0; t.modelMatrix[11] = 0; t.modelMatrix[15] = 1;   // w = x + 1
        mat4.invert(t.invModelMatrix, t.modelMatrix);
      },
    ];
    poses.forEach((pose, k) => {
      const mat = this.add_material('edge' + k, 0, [0.1, 0.6, 0.3], [0.8, 0.8, 0.8], [0, 0, 0], 0.2, 0.3, 0);
      const m = new Mesh(this.mesh_data['edge'], this.triangle_offset, this.global_id++, this.mesh_id++, this.triangle_id, mat);
      this.meshes.push(m);
      this.triangle_id += m.numTriangle;
      this.triangle_offset += m.numTriangle;
      pose(m.transform);
    });
    this.triangles = this.meshes.map(mesh => mesh.triangles).flat();   // tail of lib/scene.js create_meshes (:245-248)
    this.meshes.forEach(mesh => { mesh.calc_bbox(mesh.transform); });
    this.triangle_data = this.triangles.map(tri => tri.data);
    this.objs.push(this.meshes.flat());
  };

  const sc = new Scene();   // exact call order of renderer.js:78-87
  await sc.init_mesh_data();
  sc.create_meshes();
  save('edge', 'meshes', sc.get_meshes());
  save('edge', 'spheres', sc.get_spheres());
  save('edge', 'quads', sc.get_quads());
  save('edge', 'materials', sc.get_materials());
  save('edge', 'transforms', sc.get_transforms());
  sc.create_bvh();
  save('edge', 'bvh', sc.get_bvh());
  save('edge', 'triangles', sc.get_triangles());

  const median = BVH.create_bvh;
  BVH.create_bvh = (objs) => ({ bvh: BVH.generate_bvh_heirarchy_SAH(objs, 0, objs.length - 1), objs: objs });
  const s2 = new Scene();
  await s2.init_mesh_data();
  s2.create_meshes();
  s2.create_bvh();
  save('edgesah', 'bvh', s2.get_bvh());
  save('edgesah', 'triangles', s2.get_triangles());
  BVH.create_bvh = median;

  fs.writeFileSync(path.join(OUT, 'edge_manifest.json'), JSON.stringify(manifest, null, 1));
  console.log = say;
  console.log('wrote the edge_geometry goldens to', OUT);
}
main().catch((e) => { console.error(e); process.exit(1); });
