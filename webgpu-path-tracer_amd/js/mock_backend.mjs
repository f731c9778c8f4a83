// A recording backend with the surface of Ptmi (ptmi.mjs), for exercising the WebGPU shim without a GPU.
export class MockBackend {
  constructor() { this.calls = []; this.uploads = {}; this.frames = []; this.params = null; this.width = 0; this.height = 0; }
  setParams(p) { this.params = Object.assign({}, p); this.calls.push(['setParams']); return p; }
  upload(name, arr) { this.uploads[name] = arr; this.calls.push(['upload', name, arr.length]); }
  resize(w, h) { this.width = w; this.height = h; this.calls.push(['resize', w, h]); }
  clear() { this.calls.push(['clear']); }
  writeFramebuffer() { this.calls.push(['writeFramebuffer']); }
  renderFrame(u) { this.frames.push(Array.from(u)); this.calls.push(['renderFrame', u[2], u[3]]); }
  resolveRGBA8(fn, out) { this.calls.push(['resolve', fn]); return out || new Uint8Array(this.width * this.height * 4); }
  renderAov(views, nViews, firstFrame, framesPerView, reset = true) { this.calls.push(['renderAov', nViews, firstFrame, framesPerView, !!reset]); }
  readAov(view, layer, out) { this.calls.push(['readAov', view, layer]); return out || new Float32Array(this.width * this.height * 4); }
  releaseAov() { this.calls.push(['releaseAov']); }
  denoiseViews(frameNum, firstView, nViews, params = null) { this.calls.push(['denoiseViews', frameNum, firstView, nViews, params]); }
  denoiseViewsGuided(frameNum, firstView, nViews, params = null) { this.calls.push(['denoiseViewsGuided', frameNum, firstView, nViews, params]); }
  readDenoised(view, out) { this.calls.push(['readDenoised', view]); return out || new Float32Array(this.width * this.height * 4); }
  releaseDenoised() { this.calls.push(['releaseDenoised']); }
  fuseViews(views, frameNum, source, firstView, nViews, params = null) { this.calls.push(['fuseViews', views.length / 16, frameNum, source, firstView, nViews, params]); }
  readFused(view, out) { this.calls.push(['readFused', view]); return out || new Float32Array(this.width * this.height * 4); }
  releaseFused() { this.calls.push(['releaseFused']); }
  accumulateViews(views, frameNum, firstView, nViews, resume = false, params = null) { this.calls.push(['accumulateViews', views.length / 16, frameNum, firstView, nViews, !!resume, params]); }
  readAccumulated(view, plane, out) { this.calls.push(['readAccumulated', view, plane]); return out || new Float32Array(this.width * this.height * 4); }
  releaseAccumulated() { this.calls.push(['releaseAccumulated']); }
  denoiseViewsAccumulated(firstView, nViews, params = null) { this.calls.push(['denoiseViewsAccumulated', firstView, nViews, params]); }
  setViewMoments(on = true) { this.calls.push(['setViewMoments', on]); }
  readMoments(view, out) { this.calls.push(['readMoments', view]); return out || new Float32Array(this.width * this.height * 4); }
  releaseMoments() { this.calls.push(['releaseMoments']); }
  viewNoise(firstView, nViews, params = null) { this.calls.push(['viewNoise', firstView, nViews, params]); return Array.from({ length: nViews }, () => ({ counted: 0, sumQ: 0, above: 0, maxQ: 0 })); }
  renderViewsUntil(views, firstFrame, framesPerRound, maxFrames, target, params = null) {
    this.calls.push(['renderViewsUntil', views.length / 16, firstFrame, framesPerRound, maxFrames, target, params]);
    return { framesDone: maxFrames, noise: Array.from({ length: views.length / 16 }, () => ({ counted: 0, sumQ: 0, above: 0, maxQ: 0 })) };
  }
  denoiseViewsFrames(frameNums, firstView, nViews, params = null) { this.calls.push(['denoiseViewsFrames', Array.from(frameNums), firstView, nViews, params]); }
  denoiseViewsGuidedFrames(frameNums, firstView, nViews, params = null) { this.calls.push(['denoiseViewsGuidedFrames', Array.from(frameNums), firstView, nViews, params]); }
  fuseViewsFrames(views, frameNums, firstView, nViews, params = null) { this.calls.push(['fuseViewsFrames', views.length / 16, Array.from(frameNums), firstView, nViews, params]); }
  accumulateViewsFrames(views, frameNums, firstView, nViews, resume = false, params = null) { this.calls.push(['accumulateViewsFrames', views.length / 16, Array.from(frameNums), firstView, nViews, !!resume, params]); }
  denoiseViewsCounts(firstView, nViews, params = null) { this.calls.push(['denoiseViewsCounts', firstView, nViews, params]); }
  denoiseViewsGuidedCounts(firstView, nViews, params = null) { this.calls.push(['denoiseViewsGuidedCounts', firstView, nViews, params]); }
  fuseViewsCounts(views, firstView, nViews, params = null) { this.calls.push(['fuseViewsCounts', views.length / 16, firstView, nViews, params]); }
  accumulateViewsCounts(views, firstView, nViews, resume = false, params = null) { this.calls.push(['accumulateViewsCounts', views.length / 16, firstView, nViews, !!resume, params]); }
  accumulateViewsMotion(views, frameNums, motions, nObjects, firstView, nViews, resume = false, params = null) { this.calls.push(['accumulateViewsMotion', views.length / 16, Array.from(frameNums), motions.length / 16, nObjects, firstView, nViews, !!resume, params]); }
  captureViewGeometry(view, nViews) { this.calls.push(['captureViewGeometry', view, nViews]); }
  accumulateViewsDeform(views, frameNums, motions, nObjects, firstView, nViews, resume = false, params = null) { this.calls.push(['accumulateViewsDeform', views.length / 16, Array.from(frameNums), motions ? motions.length / 16 : null, nObjects, firstView, nViews, !!resume, params]); }
  fuseViewsMotion(views, frameNums, motions, nObjects, source, firstView, nViews, params = null) { this.calls.push(['fuseViewsMotion', views.length / 16, frameNums ? Array.from(frameNums) : null, motions.length / 16, nObjects, source, firstView, nViews, params]); }
  fuseViewsDeform(views, frameNums, motions, nObjects, source, firstView, nViews, params = null) { this.calls.push(['fuseViewsDeform', views.length / 16, frameNums ? Array.from(frameNums) : null, motions ? motions.length / 16 : null, nObjects, source, firstView, nViews, params]); }
  synchronize() {}
}
