// api_batch.cpp — the batch handle: upload, extraction (split across the aux streams),
// diagnostics, results, per-stage timing and slot packing.
#include "host.hpp"

namespace ygzfe {
// Host reads of extraction outputs: the batch stream (uploads, own launches) and the
// last extraction's end event (its descriptor pass, after every other stage joined)
// instead of a device-wide synchronisation that would also wait for unrelated streams.
// An extraction captured into a caller's graph is the caller's to synchronise.
int batch_wait(ygzfe_batch *b) {
    YGZ_HIP(hipStreamSynchronize(b->stream));
    if (b->desc_pending) YGZ_HIP(hipEventSynchronize(b->ev_desc_done));
    return YGZFE_OK;
}
}  // namespace ygzfe

static const char *kStageNames[] = {"pyramid", "blur7", "fast9_cells", "octree", "orient_rbrief", "hamming_best2",
                                    "sparse_align", "stereo", "pack_slots"};
constexpr int kNumStages = 9;

extern "C" {

// ------------------------------------------------------------------ batch
int ygzfe_batch_create(const ygzfe_orb_params *p, int device, int width, int height, int max_frames,
                       ygzfe_batch **out) {
    if (!p || !out || max_frames <= 0) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(device));
    std::unique_ptr<ygzfe_batch> b(new ygzfe_batch());
    b->p = *p;
    b->device = device;
    b->maxF = max_frames;
    YGZ_TRY(make_plan(*p, width, height, &b->plan));
    const Plan &P = b->plan->hp();
    YGZ_TRY(b->pyr.ensure((size_t)max_frames * P.pyr_bytes));
    YGZ_TRY(b->ws.ensure(P, max_frames, P.kp_cap));
    // the overflow flag ygzfe_batch_check reads: extraction clears it per call, but a batch that only
    // matches / aligns bound buffers never extracts
    YGZ_HIP(hipMemset(b->ws.err.p, 0, 16));
    YGZ_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) {
        YGZ_HIP(hipStreamCreateWithFlags(&b->aux[i], hipStreamNonBlocking));
        YGZ_HIP(hipEventCreateWithFlags(&b->ev_join[i], hipEventDisableTiming));
    }
    YGZ_HIP(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
    YGZ_HIP(hipEventCreateWithFlags(&b->ev_oct_fork, hipEventDisableTiming));
    YGZ_HIP(hipEventCreateWithFlags(&b->ev_desc_done, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) YGZ_HIP(hipEventCreateWithFlags(&b->ev_oct_join[i], hipEventDisableTiming));
    *out = b.release();
    return YGZFE_OK;
}

void ygzfe_batch_destroy(ygzfe_batch *b) {
    if (!b) return;
    std::lock_guard<std::recursive_mutex> lk(graph_mutex());
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->stream);
    (void)b->collect();
    for (auto &e : b->pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(b->stream);
    for (int i = 0; i < 3; i++) {
        if (b->aux[i]) (void)hipStreamSynchronize(b->aux[i]), (void)hipStreamDestroy(b->aux[i]);
        if (b->ev_join[i]) (void)hipEventDestroy(b->ev_join[i]);
    }
    if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
    if (b->ev_oct_fork) (void)hipEventDestroy(b->ev_oct_fork);
    if (b->ev_desc_done) (void)hipEventSynchronize(b->ev_desc_done), (void)hipEventDestroy(b->ev_desc_done);
    for (int i = 0; i < 2; i++)
        if (b->ev_oct_join[i]) (void)hipEventDestroy(b->ev_oct_join[i]);
    delete b;
}

int ygzfe_batch_info(ygzfe_batch *b, size_t *frame_pitch, int *kp_cap, int *nlevels) {
    if (!b) { set_error("null batch"); return YGZFE_EINVAL; }
    const Plan &P = b->plan->hp();
    if (frame_pitch) *frame_pitch = P.pyr_bytes;
    if (kp_cap) *kp_cap = P.kp_cap;
    if (nlevels) *nlevels = P.nlevels;
    return YGZFE_OK;
}

int ygzfe_batch_frames(ygzfe_batch *b, uint8_t **d_frames) {
    if (!b || !d_frames) { set_error("null argument"); return YGZFE_EINVAL; }
    *d_frames = b->pyr.as<uint8_t>();
    return YGZFE_OK;
}

int ygzfe_batch_bind_buffers(ygzfe_batch *b, uint8_t *d_pyramids, ygzfe_kp *d_kps, uint8_t *d_desc,
                             int32_t *d_counts) {
    if (!b) { set_error("null batch"); return YGZFE_EINVAL; }
    const Plan &P = b->plan->hp();
    YGZ_TRY(ensure_device(b->device));
    YGZ_HIP(hipStreamSynchronize(b->stream));
    if (d_pyramids) b->pyr.bind(d_pyramids, (size_t)b->maxF * P.pyr_bytes);
    if (d_kps) b->ws.kps.bind(d_kps, (size_t)b->maxF * P.kp_cap * sizeof(ygzfe_kp));
    if (d_desc) b->ws.desc.bind(d_desc, (size_t)b->maxF * P.kp_cap * 32);
    if (d_counts) b->ws.counts.bind(d_counts, (size_t)b->maxF * 4);
    return YGZFE_OK;
}

int ygzfe_batch_upload(ygzfe_batch *b, const uint8_t *frames, int n_frames) {
    if (!b || !frames || n_frames < 0 || n_frames > b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    const Plan &P = b->plan->hp();
    // the previous extraction (possibly on caller streams) may still read the slots
    if (b->desc_pending) YGZ_HIP(hipStreamWaitEvent(b->stream, b->ev_desc_done, 0));
    // frame i -> level-0 slot of pyramid i (pitch P.pyr_bytes)
    YGZ_HIP(hipMemcpy2DAsync(b->pyr.p, P.pyr_bytes, frames, (size_t)P.W * P.H, (size_t)P.W * P.H, n_frames,
                             hipMemcpyHostToDevice, b->stream));
    YGZ_HIP(hipStreamSynchronize(b->stream));
    return YGZFE_OK;
}

// Extraction as a small DAG over the launch stream and two helpers:
//   kp_stream:   pyramid -> FAST levels -> octree -> keypoint rows
//   desc_stream: (after the pyramid) GaussianBlur, concurrent with FAST;
//                (after the keypoint rows) angle + rBRIEF
// Work queued on kp_stream afterwards sees the keypoint rows (positions,
// octave, size, response; not the angle); work on desc_stream sees the
// complete rows and descriptors.
int ygzfe_batch_extract_split(ygzfe_batch *b, int n_frames, void *kp_stream, void *desc_stream) {
    if (!b || n_frames < 0 || n_frames > b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    if (n_frames == 0) return YGZFE_OK;
    YGZ_TRY(ensure_device(b->device));
    hipStream_t st = kp_stream ? (hipStream_t)kp_stream : b->stream;
    hipStream_t ds = desc_stream ? (hipStream_t)desc_stream : st;
    const PlanDev &pd = *b->plan;
    const Plan &P = pd.hp();
    Workspace &ws = b->ws;
    uint8_t *pyr = b->pyr.as<uint8_t>();
    // write-after-read across calls: the previous call's descriptor pass (on its
    // desc_stream) still reads the pyramid, blur and octree selection this call rewrites
    // (not while capturing a graph: a replay retires as a whole before the next)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    YGZ_HIP(hipStreamIsCapturing(st, &cap));
    if (b->desc_pending && cap == hipStreamCaptureStatusNone) YGZ_HIP(hipStreamWaitEvent(st, b->ev_desc_done, 0));
    YGZ_HIP(hipMemsetAsync(ws.err.p, 0, 16, st));
    // An all-area pyramid (C2: levels 1..3 exact x2 INTER_AREA) is formed by the level-0
    // blur strips as they stream level 0 (k_blur7's fused mode: level 0 read once for both),
    // on st before FAST; the other levels' blur then goes beside FAST.  (Timed as the
    // pyramid stage; YGZFE_PYR_UNFUSED=1 keeps the separate pyramid pass, for A/B.)
    static const bool unfused = getenv("YGZFE_PYR_UNFUSED") != nullptr;
    const bool fused = !unfused && pyramid_fusable(P) > 0;
    hipEvent_t t0 = b->begin(st);
    if (fused)
        YGZ_HIP(launch_pyramid_blur0(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), n_frames, st));
    else
        YGZ_HIP(launch_pyramid(pyr, P.pyr_bytes, P, pd.dp(), pd.tabs.as<int>(), n_frames, st));
    b->end(ST_PYR, t0, st);
    // the blur feeds only the descriptors: on desc_stream, beside FAST.  (Both
    // are VALU-bound; beside the octree instead, the blur slows the octree's
    // latency-bound passes by as much as it would slow FAST.)  A separate
    // stream of ygzfe's own may share the caller's hardware queue.
    hipStream_t bs = ds;
    if (ds != st) {
        YGZ_HIP(hipEventRecord(b->ev_fork, st));
        YGZ_HIP(hipStreamWaitEvent(ds, b->ev_fork, 0));
    }
    t0 = b->begin(bs);
    if (fused)
        YGZ_HIP(launch_blur_rest(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), n_frames, bs));
    else
        YGZ_HIP(launch_blur(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), n_frames, bs));
    b->end(ST_BLUR, t0, bs);
    t0 = b->begin(st);
    YGZ_HIP(launch_fast(pyr, P.pyr_bytes, P, pd.dp(), pd.cells.as<CellDesc>(), ws.cellbuf.as<uint32_t>(),
                        ws.cellcnt.as<int>(), n_frames, st));
    b->end(ST_FAST, t0, st);
    t0 = b->begin(st);
    YGZ_HIP(launch_octree(P, pd.dp(), ws.cellbuf.as<uint32_t>(), ws.cellcnt.as<int>(), ws.candA.as<uint32_t>(),
                          ws.candB.as<uint32_t>(), ws.sel.as<uint32_t>(), ws.selcnt.as<int>(), ws.err.as<int>(),
                          ws.octq.as<int>(),
                          n_frames, st, &b->aux[1], 2, b->ev_oct_fork, b->ev_oct_join));
    YGZ_HIP(launch_emit_kps(P, pd.dp(), ws.sel.as<uint32_t>(), ws.selcnt.as<int>(), nullptr, ws.kps.as<ygzfe_kp>(),
                            ws.counts.as<int>(), P.kp_cap, ws.ojobs.as<uint2>(), n_frames, st));
    b->end(ST_OCT, t0, st);
    // descriptors: after the blur (already on ds) and the keypoint rows
    if (ds != st) {
        YGZ_HIP(hipEventRecord(b->ev_join[1], st));
        YGZ_HIP(hipStreamWaitEvent(ds, b->ev_join[1], 0));
    }
    t0 = b->begin(ds);
    YGZ_HIP(launch_orient_desc(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), ws.ojobs.as<uint2>(), nullptr,
                               ws.kps.as<ygzfe_kp>(), ws.desc.as<uint8_t>(), P.kp_cap, n_frames, ds));
    b->end(ST_DESC, t0, ds);
    if (cap == hipStreamCaptureStatusNone) {
        YGZ_HIP(hipEventRecord(b->ev_desc_done, ds));
        b->desc_pending = true;
    }
    return YGZFE_OK;
}

int ygzfe_batch_extract(ygzfe_batch *b, int n_frames, void *stream) {
    // everything complete on `stream` when the last launch retires
    return ygzfe_batch_extract_split(b, n_frames, stream, stream);
}

// Measurement helper (tools/mb_fast.py): one stage alone over the first n_frames
// resident frames, `reps` back-to-back launch sets on the batch stream, average
// ms per set (hipEvents).  stage 0: FAST (writes only the cell scratch; pyramid
// levels built first when build_pyramid); stage 1: orientation + rBRIEF on the
// octree selection of the last full extraction (rewrites its angles and descriptors);
// stage 2: the GaussianBlur of every level.
int ygzfe_diag_stage_ms(ygzfe_batch *b, int stage, int n_frames, int reps, int build_pyramid, float *ms) {
    if (!b || !ms || n_frames < 1 || n_frames > b->maxF || reps < 1 || stage < 0 || stage > 2) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(b->device));
    const PlanDev &pd = *b->plan;
    const Plan &P = pd.hp();
    const uint8_t *pyr = b->pyr.as<uint8_t>();
    if (build_pyramid)
        YGZ_HIP(launch_pyramid(b->pyr.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), pd.tabs.as<int>(), n_frames, b->stream));
    hipEvent_t e0, e1;
    YGZ_HIP(hipEventCreate(&e0));
    YGZ_HIP(hipEventCreate(&e1));
    YGZ_HIP(hipEventRecord(e0, b->stream));
    Workspace &ws = b->ws;
    for (int r = 0; r < reps; r++) {
        if (stage == 0)
            YGZ_HIP(launch_fast(pyr, P.pyr_bytes, P, pd.dp(), pd.cells.as<CellDesc>(), ws.cellbuf.as<uint32_t>(),
                                ws.cellcnt.as<int>(), n_frames, b->stream));
        else if (stage == 2)
            YGZ_HIP(launch_blur(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), n_frames, b->stream));
        else
            YGZ_HIP(launch_orient_desc(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), ws.ojobs.as<uint2>(),
                                       nullptr, ws.kps.as<ygzfe_kp>(), ws.desc.as<uint8_t>(), P.kp_cap, n_frames,
                                       b->stream));
    }
    YGZ_HIP(hipEventRecord(e1, b->stream));
    YGZ_HIP(hipEventSynchronize(e1));
    YGZ_HIP(hipEventElapsedTime(ms, e0, e1));
    *ms /= reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return YGZFE_OK;
}

int ygzfe_batch_check(ygzfe_batch *b) {
    if (!b) { set_error("null batch"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    int herr = 0;
    YGZ_TRY(batch_wait(b));
    YGZ_HIP(hipMemcpy(&herr, b->ws.err.p, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) { set_error("octree node pool overflow"); return YGZFE_EINVAL; }
    return YGZFE_OK;
}

int ygzfe_batch_result(ygzfe_batch *b, int frame, ygzfe_kp *kps, int cap, uint8_t *desc, int *n_out) {
    if (!b || frame < 0 || frame >= b->maxF || !n_out) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    YGZ_TRY(batch_wait(b));
    const Plan &P = b->plan->hp();
    int n = 0;
    YGZ_HIP(hipMemcpy(&n, b->ws.counts.as<int>() + frame, sizeof(int), hipMemcpyDeviceToHost));
    *n_out = n;
    if (n > cap) { set_error("capacity %d < %d", cap, n); return YGZFE_ECAP; }
    if (kps && n) YGZ_HIP(hipMemcpy(kps, b->ws.kps.as<ygzfe_kp>() + (size_t)frame * P.kp_cap, sizeof(ygzfe_kp) * n,
                                    hipMemcpyDeviceToHost));
    if (desc && n) YGZ_HIP(hipMemcpy(desc, b->ws.desc.as<uint8_t>() + (size_t)frame * P.kp_cap * 32, (size_t)32 * n,
                                     hipMemcpyDeviceToHost));
    return YGZFE_OK;
}

int ygzfe_batch_device_results(ygzfe_batch *b, ygzfe_kp **d_kps, uint8_t **d_desc, int32_t **d_counts,
                               int *kp_cap) {
    if (!b) { set_error("null batch"); return YGZFE_EINVAL; }
    if (d_kps) *d_kps = b->ws.kps.as<ygzfe_kp>();
    if (d_desc) *d_desc = b->ws.desc.as<uint8_t>();
    if (d_counts) *d_counts = b->ws.counts.as<int32_t>();
    if (kp_cap) *kp_cap = b->plan->hp().kp_cap;
    return YGZFE_OK;
}

int ygzfe_batch_level(ygzfe_batch *b, int frame, int level, const uint8_t **d_level, int *w, int *h, int *stride) {
    if (!b || frame < 0 || frame >= b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    const Plan &P = b->plan->hp();
    if (level < 0 || level >= P.nlevels) { set_error("level out of range"); return YGZFE_EINVAL; }
    if (d_level) *d_level = b->pyr.as<uint8_t>() + (size_t)frame * P.pyr_bytes + P.lv[level].off;
    if (w) *w = P.lv[level].w;
    if (h) *h = P.lv[level].h;
    if (stride) *stride = P.lv[level].w;
    return YGZFE_OK;
}

int ygzfe_batch_read_level(ygzfe_batch *b, int frame, int level, int blurred, uint8_t *dst, int dst_stride) {
    if (!b || !dst || frame < 0 || frame >= b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    const Plan &P = b->plan->hp();
    if (level < 0 || level >= P.nlevels) { set_error("level out of range"); return YGZFE_EINVAL; }
    const LevelDesc &L = P.lv[level];
    if (dst_stride < L.w) { set_error("dst_stride < level width"); return YGZFE_EINVAL; }
    const DevBuf &src = blurred ? b->ws.blur : b->pyr;
    if (!src.p) { set_error("no %s buffer yet (run ygzfe_batch_extract first)", blurred ? "blurred" : "pyramid"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    YGZ_TRY(batch_wait(b));  // extract may have run on a caller stream + side streams
    YGZ_HIP(hipMemcpy2D(dst, dst_stride, (const uint8_t *)src.p + (size_t)frame * P.pyr_bytes + L.off, L.w, L.w, L.h,
                        hipMemcpyDeviceToHost));
    return YGZFE_OK;
}

int ygzfe_batch_stats(ygzfe_batch *b, int n_frames, int64_t *candidates, int64_t *selected) {
    if (!b || n_frames < 0 || n_frames > b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    const Plan &P = b->plan->hp();
    YGZ_TRY(ensure_device(b->device));
    YGZ_TRY(batch_wait(b));  // extract may have run on a caller stream + side streams
    for (int l = 0; l < P.nlevels; l++) {
        if (candidates) candidates[l] = 0;
        if (selected) selected[l] = 0;
    }
    if (n_frames == 0 || !b->ws.cellcnt.p) return YGZFE_OK;
    std::vector<int> cc((size_t)n_frames * P.ncells), sc((size_t)n_frames * P.nlevels);
    if (P.ncells) YGZ_HIP(hipMemcpy(cc.data(), b->ws.cellcnt.p, cc.size() * 4, hipMemcpyDeviceToHost));
    YGZ_HIP(hipMemcpy(sc.data(), b->ws.selcnt.p, sc.size() * 4, hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++)
        for (int l = 0; l < P.nlevels; l++) {
            const LevelDesc &L = P.lv[l];
            if (candidates)
                for (int c = 0; c < L.ncells; c++) candidates[l] += cc[(size_t)f * P.ncells + L.cell_begin + c];
            if (selected) selected[l] += sc[(size_t)f * P.nlevels + l];
        }
    return YGZFE_OK;
}

int ygzfe_batch_timing(ygzfe_batch *b, int enable, float *ms, const char **names, int cap) {
    if (!b) { set_error("null batch"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    YGZ_TRY(b->collect());
    for (int s = 0; s < kNumStages && s < cap; s++) {
        if (ms) ms[s] = b->calls[s] ? (float)(b->total_ms[s] / b->calls[s]) : 0.f;
        if (names) names[s] = kStageNames[s];
    }
    if (enable > 0) {  // reset + enable
        for (int s = 0; s < kNumStages; s++) { b->total_ms[s] = 0; b->calls[s] = 0; }
        b->timing = true;
    } else if (enable == 0) {
        b->timing = false;
    }
    return kNumStages;
}

void *ygzfe_batch_stream(ygzfe_batch *b) { return b ? (void *)b->stream : nullptr; }

size_t ygzfe_slot_bytes(int kp_cap) {
    if (kp_cap < 0) return 0;
    return ((size_t)YGZFE_SLOT_HEADER + (size_t)kp_cap * 60 + 15) & ~(size_t)15;
}

int ygzfe_batch_pack_slots(ygzfe_batch *b, int frame_begin, int n_frames, const struct ygzfe_align_result *d_align,
                           int global_first, uint8_t *d_slots, size_t slot_pitch, void *stream) {
    if (!b || frame_begin < 0 || n_frames < 0 || frame_begin + n_frames > b->maxF || (n_frames > 0 && !d_slots)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    const Plan &P = b->plan->hp();
    if (slot_pitch < ygzfe_slot_bytes(P.kp_cap) || (slot_pitch & 15) || ((uintptr_t)d_slots & 15)) {
        set_error("slot pitch %zu (need >= %zu, 16-B multiple, 16-B aligned base)", slot_pitch,
                  ygzfe_slot_bytes(P.kp_cap));
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(b->device));
    hipStream_t st = stream ? (hipStream_t)stream : b->stream;
    hipEvent_t t0 = b->begin(st);
    YGZ_HIP(launch_pack_slots(b->ws.kps.as<ygzfe_kp>(), b->ws.desc.as<uint8_t>(), b->ws.counts.as<int>(), P.kp_cap,
                              d_align, frame_begin, n_frames, global_first, d_slots, slot_pitch, st));
    b->end(ST_PACK, t0, st);
    return YGZFE_OK;
}

}  // extern "C"
