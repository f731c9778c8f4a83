// ptmi.mjs — loads the N-API addon (ptmi.node -> libptmi.so) and wraps it in a small class.
// There is no JavaScript fallback for rendering: if the addon or the GPU is missing, this throws.
import { createRequire } from 'module';

const require_ = createRequire(import.meta.url);
let native_ = null;

export function loadNative() {
  if (!native_) native_ = require_('./ptmi.node');
  return native_;
}

export const BUFFER_NAMES = ['spheres', 'quads', 'triangles', 'meshes', 'transforms', 'materials', 'bvh'];

// One integrator context (include/ptmi.h).  `device` is a GPU index, or an array of them: one context over several GPUs of
// the node (ptmi_create_multi) — pixel tiles sharded across them, one RCCL reduce inside readFramebuffer().
export class Ptmi {
  constructor(device = 0, native = loadNative()) {
    this.native = native;
    this.h = native.create(device);
    this.width = 0;
    this.height = 0;
  }
  destroy() { if (this.h) { this.native.destroy(this.h); this.h = null; } }
  setParams(p) { return this.native.setParams(this.h, p); }
  upload(name, typedArray) { this.native.upload(this.h, this.native.BUF[name], typedArray); }
  uploadScene(buffers) { for (const k of BUFFER_NAMES) this.upload(k, buffers[k]); }
  resize(w, h) { this.native.resize(this.h, w, h); this.width = w; this.height = h; }
  clear() { this.native.clear(this.h); }
  setShard(rank, world, tile) { this.native.setShard(this.h, rank, world, tile); }
  renderFrame(uniforms20) { this.native.renderFrame(this.h, uniforms20); }
  render(view16, firstFrame, nFrames) { this.native.render(this.h, view16, firstFrame, nFrames); }
  // A camera path in one pass (ptmi_render_views): views = Float32Array(V * 16), one column-major view matrix after the other; image v of the context's view stack
  // receives frames firstFrame .. firstFrame + framesPerView - 1 of view v (reset: a view's first frame overwrites, as resetBuffer = 1 does).
  renderViews(views, firstFrame, framesPerView, reset = true) { this.native.renderViews(this.h, views, firstFrame, framesPerView, reset); }
  readView(v, out = new Float32Array(this.width * this.height * 4)) { return this.native.readView(this.h, v, out); }
  resolveViewRGBA8(v, frameNum, out = new Uint8Array(this.width * this.height * 4)) { return this.native.resolveViewRGBA8(this.h, v, frameNum, out); }
  releaseViews() { this.native.releaseViews(this.h); }
  // The feature pass (ptmi_render_aov): views = Float32Array(nViews * 16) as for renderViews; per view three layers of width x height float4 — 0: normal sum + depth sum,
  // 1: albedo sum + hit count, 2: kind / primitive index / material index / front_face of the call's last frame — of what the first hit of every frame's path saw.
  renderAov(views, nViews, firstFrame, framesPerView, reset = true) { this.native.renderAov(this.h, views, nViews, firstFrame, framesPerView, reset); }
  readAov(view, layer, out = new Float32Array(this.width * this.height * 4)) { return this.native.readAov(this.h, view, layer, out); }
  releaseAov() { this.native.releaseAov(this.h); }
  // The denoiser (ptmi_denoise_views): filters images [firstView, firstView + nViews) of the view stack under the same images of the feature stack into the denoised
  // stack (mean radiance); frameNum = the frames each view-stack image sums; params = {levels, sigmaNormal, sigmaDepth, sigmaColour, albedoFloor}, all optional.
  denoiseViews(frameNum, firstView, nViews, params = null) { this.native.denoiseViews(this.h, frameNum, firstView, nViews, params); }
  // The variance-guided denoiser (ptmi_denoise_views_guided): denoiseViews with a luminance term scaled by the per-pixel variance of the moment stack (setViewMoments
  // must have been on while the views were rendered); writes the same denoised stack; params = {levels, sigmaNormal, sigmaDepth, sigmaLuma, albedoFloor, minFrames,
  // varEps}, all optional.
  denoiseViewsGuided(frameNum, firstView, nViews, params = null) { this.native.denoiseViewsGuided(this.h, frameNum, firstView, nViews, params); }
  readDenoised(view, out = new Float32Array(this.width * this.height * 4)) { return this.native.readDenoised(this.h, view, out); }
  releaseDenoised() { this.native.releaseDenoised(this.h); }
  // Cross-view fusion (ptmi_fuse_views): output views [firstView, firstView + nViews) gather their neighbours of the stack by reprojection into the fused stack (mean
  // radiance); views = the matrices of ALL views of the stack; source 0 = the view stack (frameNum = the frames each image sums), 1 = the denoised stack;
  // params = {radius, sigmaNormal, sigmaDepth, albedoFloor}, all optional.
  fuseViews(views, frameNum, source, firstView, nViews, params = null) { this.native.fuseViews(this.h, views, frameNum, source, firstView, nViews, params); }
  readFused(view, out = new Float32Array(this.width * this.height * 4)) { return this.native.readFused(this.h, view, out); }
  releaseFused() { this.native.releaseFused(this.h); }
  // Temporal accumulation (ptmi_accumulate_views): views [firstView, firstView + nViews) of the camera path, each on its predecessor, into the accumulated stack —
  // plane 0 mean radiance, plane 1 (D, n), plane 2 (Q, v0); views = the matrices of ALL views of the stack; resume: view firstView takes its history from view
  // firstView - 1 of the stack as it is; params = {maxHistory, minFrames, sigmaNormal, sigmaDepth, albedoFloor}, all optional.  setViewMoments must have been on
  // while the views were rendered.  denoiseViewsAccumulated: the guided filter on it, whose plane 2 brings the initial variance; writes the denoised stack.
  accumulateViews(views, frameNum, firstView, nViews, resume = false, params = null) { this.native.accumulateViews(this.h, views, frameNum, firstView, nViews, resume, params); }
  readAccumulated(view, plane, out = new Float32Array(this.width * this.height * 4)) { return this.native.readAccumulated(this.h, view, plane, out); }
  releaseAccumulated() { this.native.releaseAccumulated(this.h); }
  denoiseViewsAccumulated(firstView, nViews, params = null) { this.native.denoiseViewsAccumulated(this.h, firstView, nViews, params); }
  // Second moments and noise (ptmi_set_view_moments ...): while on, renderViews also folds the frames' squared colours (xyz) and their count (w) into the moment stack;
  // viewNoise gives per view {counted, sumQ, above, maxQ} of the pixels' relative standard error in 16.16 fixed point — mean noise = sumQ / counted / 65536;
  // renderViewsUntil renders rounds of framesPerRound frames per view until every view's mean noise is at most target or maxFrames are done:
  // {framesDone, noise}.  params = {floor, threshold}, all optional.
  setViewMoments(on = true) { this.native.setViewMoments(this.h, on); }
  readMoments(view, out = new Float32Array(this.width * this.height * 4)) { return this.native.readMoments(this.h, view, out); }
  releaseMoments() { this.native.releaseMoments(this.h); }
  viewNoise(firstView, nViews, params = null) { return this.native.viewNoise(this.h, firstView, nViews, params); }
  renderViewsUntil(views, firstFrame, framesPerRound, maxFrames, target, params = null) {
    return this.native.renderViewsUntil(this.h, views, firstFrame, framesPerRound, maxFrames, target, params);
  }
  // Per-view frame numbers and counts (ptmi_render_views_frames ...): view v gets frames firstFrames[v] .. firstFrames[v] + frameCounts[v] - 1 (Uint32Array, one entry per
  // view; a count of 0 leaves the view alone); renderViewsUntilEach stops each view once ITS mean noise is at most target: {framesDone: Uint32Array, noise}.
  renderViewsFrames(views, firstFrames, frameCounts, reset = true) { this.native.renderViewsFrames(this.h, views, firstFrames, frameCounts, reset); }
  renderAovFrames(views, firstFrames, frameCounts, reset = true) { this.native.renderAovFrames(this.h, views, firstFrames, frameCounts, reset); }
  renderViewsUntilEach(views, firstFrames, framesPerRound, maxFrames, target, params = null) {
    return this.native.renderViewsUntilEach(this.h, views, firstFrames, framesPerRound, maxFrames, target, params);
  }
  // Rendering to a noise target by runs (ptmi_render_view_runs ...): a run is 64 consecutive pixels of an image in row-major order.  renderViewRuns adds frames
  // firstFrame .. firstFrame + nFrames - 1 of view16 to image `view` of the view and moment stacks for the pixels of the listed runs alone (Uint32Array, strictly
  // ascending); viewRunNoise gives {nRuns, nOpen: Uint32Array(nViews), records: Uint32Array(nViews * nRuns * 4) — counted, sumQ, maxQ, open per run —, openRuns:
  // Uint32Array(nViews * nRuns) — per view its open runs ascending, then 0xffffffff}; renderViewsUntilRuns gives every view minFrames frames and then rounds of
  // framesPerRound to the runs that have not met target: {framesDone: Uint32Array — the most any run of the view got —, noise, pathsTraced}; readViewMean divides
  // every pixel by its own frame count (w = that count).
  renderViewRuns(view16, view, firstFrame, nFrames, runs) { this.native.renderViewRuns(this.h, view16, view, firstFrame, nFrames, Uint32Array.from(runs)); }
  // renderViewsRuns (ptmi_render_views_runs): ONE batch for the listed runs of many views — frames firstFrames[v] .. firstFrames[v] + nFrames - 1 of view v for every
  // listed view; (runViews[i], runs[i]) strictly ascending by (view, run).  views: Float32Array(16 V); the other arrays: Uint32Array or anything Uint32Array.from takes.
  renderViewsRuns(views, firstFrames, nFrames, runViews, runs) {
    this.native.renderViewsRuns(this.h, views, Uint32Array.from(firstFrames), nFrames, Uint32Array.from(runViews), Uint32Array.from(runs));
  }
  viewRunNoise(target, firstView, nViews, params = null) { return this.native.viewRunNoise(this.h, target, firstView, nViews, params); }
  renderViewsUntilRuns(views, firstFrames, framesPerRound, minFrames, maxFrames, target, params = null) {
    return this.native.renderViewsUntilRuns(this.h, views, firstFrames, framesPerRound, minFrames, maxFrames, target, params);
  }
  readViewMean(view, out = new Float32Array(this.width * this.height * 4)) { return this.native.readViewMean(this.h, view, out); }
  // The consumers with one frame count per view (ptmi_denoise_views_frames ...): frameNums = one count per view OF THE STACK, a Float32Array or anything
  // Float32Array.from takes — renderViewsUntilEach's framesDone as it is; only the entries a call reads are checked (the denoisers: the range; fusion: the range
  // widened by the radius; accumulation: the range and, resuming, the view before it).  fuseViewsFrames reads the view stack (the denoised stack holds means).
  denoiseViewsFrames(frameNums, firstView, nViews, params = null) { this.native.denoiseViewsFrames(this.h, Float32Array.from(frameNums), firstView, nViews, params); }
  denoiseViewsGuidedFrames(frameNums, firstView, nViews, params = null) { this.native.denoiseViewsGuidedFrames(this.h, Float32Array.from(frameNums), firstView, nViews, params); }
  fuseViewsFrames(views, frameNums, firstView, nViews, params = null) { this.native.fuseViewsFrames(this.h, views, Float32Array.from(frameNums), firstView, nViews, params); }
  accumulateViewsFrames(views, frameNums, firstView, nViews, resume = false, params = null) {
    this.native.accumulateViewsFrames(this.h, views, Float32Array.from(frameNums), firstView, nViews, resume, params);
  }
  // Per-pixel frame counts (ptmi_denoise_views_counts ...): the consumers for a stack whose PIXELS differ in frame count (renderViewRuns, renderViewsRuns,
  // renderViewsUntilRuns).  Every pixel's divisor is its own M.w in the moment stack, read on the device: no count argument.  setViewMoments must have been on.
  denoiseViewsCounts(firstView, nViews, params = null) { this.native.denoiseViewsCounts(this.h, firstView, nViews, params); }
  denoiseViewsGuidedCounts(firstView, nViews, params = null) { this.native.denoiseViewsGuidedCounts(this.h, firstView, nViews, params); }
  fuseViewsCounts(views, firstView, nViews, params = null) { this.native.fuseViewsCounts(this.h, views, firstView, nViews, params); }
  accumulateViewsCounts(views, firstView, nViews, resume = false, params = null) { this.native.accumulateViewsCounts(this.h, views, firstView, nViews, resume, params); }
  // ptmi_accumulate_views_motion: motions holds, per view of the stack and object (global_id), the column-major matrix that carries a world point of the object at
  // the time of view v to the same material point at the time of view v - 1: Float32Array [view][object][16]
  accumulateViewsMotion(views, frameNums, motions, nObjects, firstView, nViews, resume = false, params = null) {
    this.native.accumulateViewsMotion(this.h, views, Float32Array.from(frameNums), motions, nObjects, firstView, nViews, resume, params);
  }
  // ptmi_capture_view_geometry: the device triangles in the order they lie in now and the transform table as uploaded now, into slot `view` of the context's
  // geometry stack of nViews slots — after refitSceneBVH and the view's render, before the next upload
  captureViewGeometry(view, nViews) { this.native.captureViewGeometry(this.h, view, nViews); }
  // ptmi_accumulate_views_deform: accumulateViewsMotion through the geometry stack — a triangle pixel is carried from its triangle in view v to the same triangle in
  // view v - 1; motions (null with nObjects 0: a static world) serve every other pixel
  accumulateViewsDeform(views, frameNums, motions, nObjects, firstView, nViews, resume = false, params = null) {
    this.native.accumulateViewsDeform(this.h, views, Float32Array.from(frameNums), motions, nObjects, firstView, nViews, resume, params);
  }
  // ptmi_fuse_views_motion: fuseViewsFrames through a world whose objects move — motions as accumulateViewsMotion takes them, composed across each output view's
  // window by the library; source 1 reads the denoised stack, frameNums may then be null
  fuseViewsMotion(views, frameNums, motions, nObjects, source, firstView, nViews, params = null) {
    this.native.fuseViewsMotion(this.h, views, frameNums == null ? null : Float32Array.from(frameNums), motions, nObjects, source, firstView, nViews, params);
  }
  // ptmi_fuse_views_deform: fuseViewsMotion through the geometry stack — a triangle pixel is carried from its triangle in view v to the same triangle in every view
  // of its window; motions (null with nObjects 0: a static world) serve every other pixel
  fuseViewsDeform(views, frameNums, motions, nObjects, source, firstView, nViews, params = null) {
    this.native.fuseViewsDeform(this.h, views, frameNums == null ? null : Float32Array.from(frameNums), motions, nObjects, source, firstView, nViews, params);
  }
  synchronize() { this.native.synchronize(this.h); }
  prepare() { this.native.prepare(this.h); }
  buildSceneBVHSAH() { this.native.buildSceneBVHSAH(this.h); }   // the same with the reference's never-called SAH builder (lib/BVH/bvhNode.js:108-283): opt-in
  refitSceneBVH() { this.native.refitSceneBVH(this.h); }   // ptmi_refit_scene_bvh: the device-resident tree's boxes recomputed over what is uploaded now (moved triangles / transforms), no rebuild
  buildSceneBVH() { this.native.buildSceneBVH(this.h); }   // Scene.create_bvh() (lib/scene.js:253-259) on the GPU, over the uploaded unordered triangles
  readFramebuffer(out = new Float32Array(this.width * this.height * 4)) { return this.native.readFramebuffer(this.h, out); }
  writeFramebuffer(src) { this.native.writeFramebuffer(this.h, src); }
  resolveRGBA8(frameNum, out = new Uint8Array(this.width * this.height * 4)) { return this.native.resolveRGBA8(this.h, frameNum, out); }
  setCounters(on) { this.native.setCounters(this.h, on); }
  setTiming(on) { this.native.setTiming(this.h, on); }
  stats() { return this.native.stats(this.h); }
  resetStats() { this.native.resetStats(this.h); }
}
