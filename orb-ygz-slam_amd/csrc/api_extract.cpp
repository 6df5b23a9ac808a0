// api_extract.cpp — extractor and frame handles, pyramid and level I/O, and the single-frame
// extraction (ygzfe_extract: forked side streams, captured once per frame handle as a graph).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "host.hpp"

int ygzfe_extractor::ensure_side() {
    if (side[0]) return YGZFE_OK;
    for (int i = 0; i < 3; i++) {
        YGZ_HIP(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
        YGZ_HIP(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
    }
    YGZ_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    YGZ_HIP(hipEventCreateWithFlags(&ev_oct_fork, hipEventDisableTiming));
    YGZ_HIP(hipEventCreateWithFlags(&ev_img, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) YGZ_HIP(hipEventCreateWithFlags(&ev_oct_join[i], hipEventDisableTiming));
    return YGZFE_OK;
}

namespace ygzfe {
int pyramid_from_level0(ygzfe_frame *f, hipStream_t st) {
    const PlanDev &pd = *f->plan;
    YGZ_HIP(launch_pyramid(f->pyr.as<uint8_t>(), pd.hp().pyr_bytes, pd.hp(), pd.dp(), pd.tabs.as<int>(), 1, st));
    return YGZFE_OK;
}
}  // namespace ygzfe

static inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" {

// ------------------------------------------------------------------ extractor
int ygzfe_extractor_create(const ygzfe_orb_params *p, int device, ygzfe_extractor **out) {
    if (!p || !out) { set_error("null argument"); return YGZFE_EINVAL; }
    if (p->nlevels < 1 || p->nlevels > YGZFE_MAX_LEVELS || !(p->scale_factor > 1.0f) || p->nfeatures < 0) {
        set_error("invalid ORB parameters");
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(device));
    std::unique_ptr<ygzfe_extractor> ex(new ygzfe_extractor());
    ex->p = *p;
    ex->device = device;
    orb_scales(*p, &ex->scales);
    YGZ_HIP(hipStreamCreateWithFlags(&ex->stream, hipStreamNonBlocking));
    *out = ex.release();
    return YGZFE_OK;
}

static void extractor_release(ygzfe_extractor *ex) {
    (void)hipSetDevice(ex->device);
    if (ex->stream) (void)hipStreamSynchronize(ex->stream);
    for (int i = 0; i < 3; i++) {
        if (ex->side[i]) (void)hipStreamSynchronize(ex->side[i]), (void)hipStreamDestroy(ex->side[i]);
        if (ex->ev_join[i]) (void)hipEventDestroy(ex->ev_join[i]);
    }
    if (ex->ev_fork) (void)hipEventDestroy(ex->ev_fork);
    if (ex->astream) {
        (void)hipStreamSynchronize(ex->astream);
        (void)hipStreamDestroy(ex->astream);
        (void)hipEventDestroy(ex->ev_align_fork);
        (void)hipEventDestroy(ex->ev_align_done);
    }
    if (ex->ev_img) (void)hipEventDestroy(ex->ev_img);
    if (ex->ev_oct_fork) (void)hipEventDestroy(ex->ev_oct_fork);
    for (int i = 0; i < 2; i++)
        if (ex->ev_oct_join[i]) (void)hipEventDestroy(ex->ev_oct_join[i]);
    ex->plans.clear();
    if (ex->stream) (void)hipStreamDestroy(ex->stream);
    delete ex;
}

void ygzfe_extractor_destroy(ygzfe_extractor *ex) {
    if (!ex) return;
    std::lock_guard<std::recursive_mutex> lk(graph_mutex());
    if (ex->live_frames > 0) {  // released by the last frame (a finalizer order we do not control)
        ex->dead = true;
        return;
    }
    extractor_release(ex);
}

int ygzfe_orb_plan(const ygzfe_orb_params *p, int width, int height, int32_t *level_w, int32_t *level_h,
                   int32_t *budget, int32_t *ncells, int32_t *umax) {
    if (!p) { set_error("null argument"); return YGZFE_EINVAL; }
    PlanHost ph;
    char err[256];
    if (build_plan(*p, width, height, &ph, err, sizeof(err)) != 0) { set_error("%s", err); return YGZFE_EINVAL; }
    for (int l = 0; l < ph.plan.nlevels; l++) {
        if (level_w) level_w[l] = ph.plan.lv[l].w;
        if (level_h) level_h[l] = ph.plan.lv[l].h;
        if (budget) budget[l] = ph.plan.lv[l].budget;
        if (ncells) ncells[l] = ph.plan.lv[l].ncells;
    }
    if (umax)
        for (int i = 0; i < 16; i++) umax[i] = ph.plan.umax[i];
    return YGZFE_OK;
}

int ygzfe_orb_plan_choices(const ygzfe_orb_params *p, int width, int height, int32_t *per_level, int32_t *per_plan) {
    if (!p) { set_error("null argument"); return YGZFE_EINVAL; }
    PlanHost ph;
    char err[256];
    if (build_plan(*p, width, height, &ph, err, sizeof(err)) != 0) { set_error("%s", err); return YGZFE_EINVAL; }
    const Plan &P = ph.plan;
    for (int l = 0; l < P.nlevels && per_level; l++) {
        const LevelDesc &L = P.lv[l];
        int32_t *o = per_level + (size_t)l * YGZFE_PLAN_LEVEL_FIELDS;
        int S = 0, R = 0;
        if (L.ncells > 0) fast_shape_pick(L.fast_rw, L.fast_rh, S, R);  // launch_fast skips a level without cells
        const int nc = octree_nc(L);
        const int32_t row[YGZFE_PLAN_LEVEL_FIELDS] = {L.n_ini, L.oct_rb, L.ncells, L.fast_rw, L.fast_rh, nc, S, R,
                                                      octree_sort0_keys(nc, false), octree_sort0_keys(nc, true)};
        memcpy(o, row, sizeof(row));
    }
    if (per_plan) {
        int S = 0, R = 0;
        if (P.ncells > 0) fast_shape_merged(P, S, R);
        per_plan[0] = S;
        per_plan[1] = R;
        per_plan[2] = octree_groups(P);
    }
    return YGZFE_OK;
}

int ygzfe_extractor_levels(const ygzfe_extractor *ex, int *nlevels, float *scale, float *inv_scale,
                           float *sigma2, float *inv_sigma2) {
    if (!ex) { set_error("null extractor"); return YGZFE_EINVAL; }
    const int L = ex->p.nlevels;
    if (nlevels) *nlevels = L;
    for (int i = 0; i < L; i++) {
        if (scale) scale[i] = ex->scales.scale[i];
        if (inv_scale) inv_scale[i] = ex->scales.inv_scale[i];
        if (sigma2) sigma2[i] = ex->scales.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = ex->scales.inv_sigma2[i];
    }
    return YGZFE_OK;
}

int ygzfe_extractor_features_per_level(const ygzfe_extractor *ex, int32_t *out) {
    if (!ex || !out) { set_error("null argument"); return YGZFE_EINVAL; }
    for (int i = 0; i < ex->p.nlevels; i++) out[i] = ex->scales.budget[i];
    return YGZFE_OK;
}

int ygzfe_extractor_dso_grid(ygzfe_extractor *ex, int32_t *get, const int32_t *set) {
    if (!ex) { set_error("null extractor"); return YGZFE_EINVAL; }
    if (get) *get = ex->dso_grid;
    if (set) ex->dso_grid = *set;
    return YGZFE_OK;
}

static int extractor_plan(ygzfe_extractor *ex, int W, int H, PlanDev **out) {
    auto key = std::make_pair(W, H);
    auto it = ex->plans.find(key);
    if (it == ex->plans.end()) {
        std::unique_ptr<PlanDev> pd;
        YGZ_TRY(make_plan(ex->p, W, H, &pd));
        it = ex->plans.emplace(key, std::move(pd)).first;
    }
    *out = it->second.get();
    return YGZFE_OK;
}

int ygzfe_frame_create(ygzfe_extractor *ex, int width, int height, ygzfe_frame **out) {
    if (!ex || !out) { set_error("null argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    std::unique_ptr<ygzfe_frame> f(new ygzfe_frame());
    f->ex = ex;
    f->W = width;
    f->H = height;
    YGZ_TRY(extractor_plan(ex, width, height, &f->plan));
    YGZ_TRY(f->pyr.ensure(f->plan->hp().pyr_bytes));
    {
        std::lock_guard<std::recursive_mutex> g(graph_mutex());
        ex->live_frames++;
    }
    *out = f.release();
    return YGZFE_OK;
}

void ygzfe_frame_destroy(ygzfe_frame *f) {
    if (!f) return;
    (void)hipSetDevice(f->ex->device);
    {
        // an alignment in flight (ygzfe_sparse_align_begin, on ex->astream) may read this
        // frame's pyramid: wait for it (its result stays staged for _end)
        std::lock_guard<std::mutex> lk(f->ex->mu);
        if (f->ex->align_pending) (void)hipEventSynchronize(f->ex->ev_align_done);
        (void)hipStreamSynchronize(f->ex->stream);
    }
    std::lock_guard<std::recursive_mutex> lk(graph_mutex());
    ygzfe_extractor *ex = f->ex;
    delete f;
    if (--ex->live_frames == 0 && ex->dead) extractor_release(ex);
}

int ygzfe_compute_pyramid(ygzfe_extractor *ex, ygzfe_frame *f, const uint8_t *img, int stride) {
    if (!ex || !f || !img || stride < f->W) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    f->n_kps = -1;  // keypoints belong to the image they were set for
    // the image is copied into pinned staging (the caller may reuse `img` at once)
    // and DMA'd from there; everything that reads the pyramid is ordered after it
    // on ex->stream or synchronises first (ygzfe_frame_level), so no
    // synchronisation here -- only before the staging is overwritten
    YGZ_TRY(ex->ensure_side());
    const size_t n = (size_t)f->W * f->H;
    YGZ_HIP(hipEventSynchronize(ex->ev_img));  // the previous DMA out of himg (before it may be reallocated)
    YGZ_TRY(ex->order_after_align(ex->stream));
    YGZ_TRY(ex->himg.ensure(n));
    uint8_t *h = ex->himg.as<uint8_t>();
    if (stride == f->W) {
        memcpy(h, img, n);
    } else {
        for (int y = 0; y < f->H; y++) memcpy(h + (size_t)y * f->W, img + (size_t)y * stride, (size_t)f->W);
    }
    YGZ_HIP(hipMemcpyAsync(f->pyr.p, h, n, hipMemcpyHostToDevice, ex->stream));
    YGZ_HIP(hipEventRecord(ex->ev_img, ex->stream));
    YGZ_TRY(pyramid_from_level0(f, ex->stream));
    return YGZFE_OK;
}

int ygzfe_compute_pyramid_device(ygzfe_extractor *ex, ygzfe_frame *f, const uint8_t *d_img, int stride,
                                 void *stream) {
    if (!ex || !f || !d_img || stride < f->W) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(ex->device));
    f->n_kps = -1;
    hipStream_t st = stream ? (hipStream_t)stream : ex->stream;
    YGZ_TRY(ex->order_after_align(st));
    YGZ_HIP(hipMemcpy2DAsync(f->pyr.p, f->W, d_img, stride, f->W, f->H, hipMemcpyDeviceToDevice, st));
    YGZ_TRY(pyramid_from_level0(f, st));
    if (!stream) YGZ_HIP(hipStreamSynchronize(st));
    return YGZFE_OK;
}

int ygzfe_frame_level(const ygzfe_frame *f, int level, int *w, int *h, uint8_t *dst, int dst_stride) {
    if (!f) { set_error("null frame"); return YGZFE_EINVAL; }
    const Plan &P = f->plan->hp();
    if (level < 0 || level >= P.nlevels) { set_error("level %d out of range", level); return YGZFE_EINVAL; }
    const LevelDesc &L = P.lv[level];
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (dst) {
        if (dst_stride < L.w) { set_error("dst_stride < level width"); return YGZFE_EINVAL; }
        ygzfe_extractor *ex = f->ex;
        YGZ_TRY(ensure_device(ex->device));
        std::lock_guard<std::mutex> lk(ex->mu);
        // one contiguous DMA into page-locked staging, ordered after the frame's work on
        // ex->stream, then the row copy on the host
        const size_t n = (size_t)L.w * L.h;
        YGZ_HIP(hipStreamSynchronize(ex->stream));  // the staging's previous use, the pyramid's writers
        YGZ_TRY(ex->hlvl.ensure(n));
        YGZ_HIP(hipMemcpyAsync(ex->hlvl.p, f->pyr.as<uint8_t>() + L.off, n, hipMemcpyDeviceToHost, ex->stream));
        YGZ_HIP(hipStreamSynchronize(ex->stream));
        const uint8_t *hs = ex->hlvl.as<uint8_t>();
        if (dst_stride == L.w) {
            memcpy(dst, hs, n);
        } else {
            for (int y = 0; y < L.h; y++) memcpy(dst + (size_t)y * dst_stride, hs + (size_t)y * L.w, (size_t)L.w);
        }
    }
    return YGZFE_OK;
}

int ygzfe_frame_set_level(ygzfe_frame *f, int level, const uint8_t *src, int src_stride) {
    if (!f || !src) { set_error("null argument"); return YGZFE_EINVAL; }
    const Plan &P = f->plan->hp();
    if (level < 0 || level >= P.nlevels) { set_error("level %d out of range", level); return YGZFE_EINVAL; }
    const LevelDesc &L = P.lv[level];
    if (src_stride < L.w) { set_error("src_stride < level width"); return YGZFE_EINVAL; }
    ygzfe_extractor *ex = f->ex;
    f->n_kps = -1;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    YGZ_HIP(hipStreamSynchronize(ex->stream));  // the staging's previous use
    if (ex->align_pending) YGZ_HIP(hipEventSynchronize(ex->ev_align_done));  // an alignment reading this pyramid
    const size_t n = (size_t)L.w * L.h;
    YGZ_TRY(ex->hlvl.ensure(n));
    uint8_t *hs = ex->hlvl.as<uint8_t>();
    if (src_stride == L.w) {
        memcpy(hs, src, n);
    } else {
        for (int y = 0; y < L.h; y++) memcpy(hs + (size_t)y * L.w, src + (size_t)y * src_stride, (size_t)L.w);
    }
    YGZ_HIP(hipMemcpyAsync(f->pyr.as<uint8_t>() + L.off, hs, n, hipMemcpyHostToDevice, ex->stream));
    YGZ_HIP(hipStreamSynchronize(ex->stream));  // the level is in place when the call returns, as before
    return YGZFE_OK;
}

// levels [first, first + count) of the plan: checked range, and the device span
// [lv[first].off, lv[last].off + w * h) that holds them (one DMA for all)
static int level_span(const ygzfe_frame *f, int first, int count, size_t *off, size_t *bytes) {
    const Plan &P = f->plan->hp();
    if (first < 0 || count < 1 || first + count > P.nlevels) {
        set_error("levels [%d, %d) out of range (%d levels)", first, first + count, P.nlevels);
        return YGZFE_EINVAL;
    }
    const LevelDesc &a = P.lv[first], &b = P.lv[first + count - 1];
    *off = a.off;
    *bytes = (size_t)b.off + (size_t)b.w * b.h - a.off;
    return YGZFE_OK;
}

int ygzfe_frame_levels(const ygzfe_frame *f, int first, int count, uint8_t *const *dst, const int *dst_stride) {
    if (!f || !dst || !dst_stride) { set_error("null argument"); return YGZFE_EINVAL; }
    size_t off = 0, bytes = 0;
    YGZ_TRY(level_span(f, first, count, &off, &bytes));
    const Plan &P = f->plan->hp();
    for (int i = 0; i < count; i++)
        if (!dst[i] || dst_stride[i] < P.lv[first + i].w) { set_error("level %d: no buffer or stride < width", first + i); return YGZFE_EINVAL; }
    ygzfe_extractor *ex = f->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    // every level in one DMA into page-locked staging, ordered after the pyramid's writers on
    // ex->stream; one synchronisation, then the row copies on the host
    // (every user of the staging synchronises before it returns, under ex->mu)
    YGZ_TRY(ex->hlvl.ensure(bytes));
    YGZ_HIP(hipMemcpyAsync(ex->hlvl.p, f->pyr.as<uint8_t>() + off, bytes, hipMemcpyDeviceToHost, ex->stream));
    YGZ_HIP(hipStreamSynchronize(ex->stream));
    for (int i = 0; i < count; i++) {
        const LevelDesc &L = P.lv[first + i];
        const uint8_t *hs = ex->hlvl.as<uint8_t>() + (L.off - off);
        if (dst_stride[i] == L.w) {
            memcpy(dst[i], hs, (size_t)L.w * L.h);
        } else {
            for (int y = 0; y < L.h; y++) memcpy(dst[i] + (size_t)y * dst_stride[i], hs + (size_t)y * L.w, (size_t)L.w);
        }
    }
    return YGZFE_OK;
}

int ygzfe_frame_set_levels(ygzfe_frame *f, int first, int count, const uint8_t *const *src, const int *src_stride) {
    if (!f || !src || !src_stride) { set_error("null argument"); return YGZFE_EINVAL; }
    size_t off = 0, bytes = 0;
    YGZ_TRY(level_span(f, first, count, &off, &bytes));
    const Plan &P = f->plan->hp();
    for (int i = 0; i < count; i++)
        if (!src[i] || src_stride[i] < P.lv[first + i].w) { set_error("level %d: no buffer or stride < width", first + i); return YGZFE_EINVAL; }
    f->n_kps = -1;
    ygzfe_extractor *ex = f->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    if (ex->align_pending) YGZ_HIP(hipEventSynchronize(ex->ev_align_done));  // an alignment reading this pyramid
    // no DMA may still target the staging (an earlier call that returned on an error
    // between its async copy and its synchronisation), as in ygzfe_frame_set_level
    YGZ_HIP(hipStreamSynchronize(ex->stream));
    YGZ_TRY(ex->hlvl.ensure(bytes));
    for (int i = 0; i < count; i++) {
        const LevelDesc &L = P.lv[first + i];
        uint8_t *hs = ex->hlvl.as<uint8_t>() + (L.off - off);
        if (src_stride[i] == L.w) {
            memcpy(hs, src[i], (size_t)L.w * L.h);
        } else {
            for (int y = 0; y < L.h; y++) memcpy(hs + (size_t)y * L.w, src[i] + (size_t)y * src_stride[i], (size_t)L.w);
        }
    }
    // the gaps between levels carry staging bytes: no kernel reads them as pixels
    YGZ_HIP(hipMemcpyAsync(f->pyr.as<uint8_t>() + off, ex->hlvl.p, bytes, hipMemcpyHostToDevice, ex->stream));
    YGZ_HIP(hipStreamSynchronize(ex->stream));  // the levels are in place when the call returns
    return YGZFE_OK;
}

static int dso_max_rows(const Plan &P) {
    const int g = 7;
    return 3 * (P.lv[0].w / g) * (P.lv[0].h / g);
}

// YGZFE_TRACE=1 (debugging): ygzfe_extract's steps on stderr
static void trace_step(const char *what, long a = 0, long b = 0) {
    static const bool on = getenv("YGZFE_TRACE") != nullptr;
    if (on) {
        fprintf(stderr, "[ygzfe_extract] %s %ld %ld\n", what, a, b);
        fflush(stderr);
    }
}

int ygzfe_extract(ygzfe_extractor *ex, ygzfe_frame *f, int method, ygzfe_kp *kps_io, int n_existing, int cap,
                  uint8_t *desc, int *n_out) {
    trace_step("enter", method, cap);
    if (!ex || !f || !n_out || n_existing < 0 || (n_existing > 0 && !kps_io)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (method == YGZFE_FAST_KEYPOINT) {
        set_error("FAST_KEYPOINT is flagged buggy and never called by the reference (ORBextractor.cc:1191)");
        return YGZFE_EINVAL;
    }
    if (method != YGZFE_ORBSLAM_KEYPOINT && method != YGZFE_DSO_KEYPOINT) {
        set_error("unknown method %d", method);
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    const PlanDev &pd = *f->plan;
    const Plan &P = pd.hp();
    hipStream_t st = ex->stream;
    const int rows = n_existing + (method == YGZFE_DSO_KEYPOINT ? std::max(P.kp_cap, dso_max_rows(P)) : P.kp_cap);
    Workspace &ws = ex->ws;
    YGZ_TRY(ws.ensure(P, 1, rows));
    trace_step("workspace", rows, P.kp_cap);
    const uint8_t *pyr = f->pyr.as<uint8_t>();
    int total = 0;
    if (method == YGZFE_ORBSLAM_KEYPOINT) {
        // The single-frame DAG (one Tracking thread's latency): the blur on side[0]
        // beside FAST (st); the octree on st (its node-pool classes in sequence, or with
        // YGZFE_OCT_FORK the classes after the first on side[1]); keypoint rows, angle +
        // rBRIEF after the blur's join; one packing kernel, one D2H into pinned memory,
        // one synchronisation.  Every stream forked here is joined back into st before
        // the capture ends (checked after every capture).
        YGZ_TRY(ex->ensure_side());
        // The rows, descriptors, count and octree-overflow flag are written straight
        // into one result buffer -- [count, flag, 0, 0][rows x 28 B keypoints]
        // [16-B aligned: rows x 32 B descriptors] -- so one D2H returns everything.
        const size_t kbytes = align16(sizeof(ygzfe_kp) * (size_t)rows), rbytes = 16 + kbytes + (size_t)32 * rows;
        YGZ_TRY(ex->res.ensure(rbytes));
        YGZ_TRY(ex->hout.ensure(rbytes));
        uint8_t *res = ex->res.as<uint8_t>();
        int *d_count = reinterpret_cast<int *>(res), *d_err = d_count + 1;
        ygzfe_kp *d_kps = reinterpret_cast<ygzfe_kp *>(res + 16);
        uint8_t *d_desc = res + 16 + kbytes;
        const int *d_nexist = nullptr;  // null: no existing rows (the kernels read 0)
        if (n_existing > 0) {
            YGZ_TRY(ex->hin.ensure(16 + sizeof(ygzfe_kp) * (size_t)n_existing));
            ex->hin.as<int>()[0] = n_existing;
            memcpy(ex->hin.as<uint8_t>() + 16, kps_io, sizeof(ygzfe_kp) * n_existing);
            YGZ_HIP(hipMemcpyAsync(ws.nexist.p, ex->hin.p, sizeof(int), hipMemcpyHostToDevice, st));
            YGZ_HIP(hipMemcpyAsync(d_kps, ex->hin.as<uint8_t>() + 16, sizeof(ygzfe_kp) * n_existing,
                                   hipMemcpyHostToDevice, st));
            d_nexist = ws.nexist.as<int>();
        }
        // the header and, speculatively, as many rows as the caller can take (one DMA)
        const int cap_rows = std::min(rows, std::max(cap, 0));
        const size_t copy = desc ? 16 + kbytes + (size_t)32 * cap_rows : 16 + sizeof(ygzfe_kp) * (size_t)cap_rows;
        hipStream_t *sd = ex->side;
        // the DAG: blur on side[0] beside FAST (every level in one launch; its first
        // lane also clears the overflow flag) on st; the octree; rows + jobs, then
        // angle + rBRIEF after the blur joins; the D2H.  Only side[0] waits on ev_fork:
        // round 5 forked all three side streams here and joined only side[0], and a
        // capture of that crashed inside hipGraphLaunch (profiles/r05_graph_fork.txt).
        static const bool oct_fork = getenv("YGZFE_OCT_FORK") != nullptr;
        auto enqueue = [&]() -> int {
            YGZ_HIP(hipEventRecord(ex->ev_fork, st));
            YGZ_HIP(hipStreamWaitEvent(sd[0], ex->ev_fork, 0));
            YGZ_HIP(launch_blur(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), 1, sd[0]));
            YGZ_HIP(hipEventRecord(ex->ev_join[0], sd[0]));
            YGZ_HIP(launch_fast_merged(pyr, P.pyr_bytes, P, pd.dp(), pd.cells.as<CellDesc>(),
                                       ws.cellbuf.as<uint32_t>(), ws.cellcnt.as<int>(), 1, st, d_err));
            // the node-pool classes (nfeatures > ~1000 puts level 0 in a larger class than
            // the rest): in sequence on st, or forked onto side[1] (launch_octree records
            // its own fork event after FAST and joins side[1] back before it returns)
            YGZ_HIP(launch_octree(P, pd.dp(), ws.cellbuf.as<uint32_t>(), ws.cellcnt.as<int>(), ws.candA.as<uint32_t>(),
                                  ws.candB.as<uint32_t>(), ws.sel.as<uint32_t>(), ws.selcnt.as<int>(), d_err,
                                  ws.octq.as<int>(), 1, st, oct_fork ? &sd[1] : nullptr, oct_fork ? 1 : 0,
                                  ex->ev_oct_fork, ex->ev_oct_join, true));
            YGZ_HIP(launch_emit_kps(P, pd.dp(), ws.sel.as<uint32_t>(), ws.selcnt.as<int>(), d_nexist, d_kps, d_count,
                                    rows, ws.ojobs.as<uint2>(), 1, st));
            YGZ_HIP(hipStreamWaitEvent(st, ex->ev_join[0], 0));  // the blurred levels
            YGZ_HIP(launch_orient_desc(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), ws.ojobs.as<uint2>(),
                                       d_nexist, d_kps, d_desc, rows, 1, st));
            YGZ_HIP(launch_desc_existing(pyr, ws.blur.as<uint8_t>(), pd.dp(), d_kps, d_desc, n_existing, 0, st));
            YGZ_HIP(hipMemcpyAsync(ex->hout.p, res, copy, hipMemcpyDeviceToHost, st));
            return YGZFE_OK;
        };
        // Without existing rows the whole sequence (9-12 launches, the event fork /
        // joins and the D2H) is replayed from a HIP graph captured once per frame
        // handle: one submission instead of one host call per launch.  The graph is
        // re-captured when any buffer it names has moved or the copy size changed.
        const void *key[15] = {pyr,          ws.blur.p,  ws.cellbuf.p, ws.sel.p,       ws.candA.p,
                               ws.candB.p,   ex->res.p,  ex->hout.p,   ws.ojobs.p,     ws.cellcnt.p,
                               ws.selcnt.p,  pd.cells.p, pd.plan.p,    pd.tabs.p,      ws.octq.p};
        static_assert(sizeof(key) == sizeof(f->gkey), "graph key size");
        static const bool no_graph = getenv("YGZFE_NO_GRAPH") != nullptr;
        bool launched = false;
        trace_step("staged", (long)rbytes, (long)copy);
        if (n_existing == 0 && !no_graph && !ex->graph_broken) {
            if (!f->gexec || memcmp(f->gkey, key, sizeof(key)) != 0 || f->grows != rows || f->gcopy != copy) {
                trace_step("capture", (long)(f->gexec != nullptr), 0);
                std::lock_guard<std::recursive_mutex> lk(graph_mutex());
                f->drop_graph();
                bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
                const int rc = ok ? enqueue() : YGZFE_EHIP;
                hipGraph_t g = nullptr;
                if (ok) ok = hipStreamEndCapture(st, &g) == hipSuccess && rc == YGZFE_OK && g;
                f->graph = g;
                // a stream still capturing after the origin's EndCapture is an unjoined fork:
                // its next launch would land in this graph, freed by the next drop_graph()
                const int bad = ex->capture_left_open();
                if (bad >= 0) {
                    f->drop_graph();
                    ex->graph_broken = true;
                    (void)hipGetLastError();
                    set_error("stream %d still capturing after ygzfe_extract's capture ended", bad);
                    return YGZFE_EHIP;
                }
                if (ok) ok = hipGraphInstantiate(&f->gexec, g, nullptr, nullptr, 0) == hipSuccess;
                if (ok) {
                    memcpy(f->gkey, key, sizeof(key));
                    f->grows = rows;
                    f->gcopy = copy;
                } else {  // capture unsupported here: plain launches from now on
                    f->drop_graph();
                    ex->graph_broken = true;
                    (void)hipGetLastError();
                }
            }
            if (f->gexec) {
                YGZ_HIP(hipGraphLaunch(f->gexec, st));
                launched = true;
            }
        }
        trace_step("launched", launched, 0);
        if (!launched) YGZ_TRY(enqueue());
        YGZ_HIP(hipStreamSynchronize(st));
        total = ex->hout.as<int>()[0];
        trace_step("synced", total, ex->hout.as<int>()[1]);
        if (ex->hout.as<int>()[1]) {
            set_error("octree node pool overflow");
            return YGZFE_EINVAL;
        }
        *n_out = total;
        if (total > cap) {
            set_error("capacity %d < %d keypoints", cap, total);
            return YGZFE_ECAP;
        }
        if (total > 0) {
            memcpy(kps_io, ex->hout.as<uint8_t>() + 16, sizeof(ygzfe_kp) * (size_t)total);
            if (desc) memcpy(desc, ex->hout.as<uint8_t>() + 16 + kbytes, (size_t)32 * total);
        }
        return YGZFE_OK;
    } else {
        if (n_existing > 0)
            YGZ_HIP(hipMemcpyAsync(ws.kps.p, kps_io, sizeof(ygzfe_kp) * n_existing, hipMemcpyHostToDevice, st));
        YGZ_HIP(launch_blur(pyr, ws.blur.as<uint8_t>(), P.pyr_bytes, P, pd.dp(), 1, st));
        // DSO_KEYPOINT: ComputeKeyPointsDSOSingleLevel (ORBextractor.cc:1275-1386)
        const LevelDesc &L0 = P.lv[0];
        const int w = L0.w, h = L0.h, n = ex->p.nfeatures;
        YGZ_TRY(ws.occ.ensure((size_t)w * h));
        YGZ_HIP(launch_dso_occupancy(ws.kps.as<ygzfe_kp>(), n_existing, ws.occ.as<uint8_t>(), w, h, st));
        int g = ex->dso_grid;
        if (g < 0) g = (int)sqrt(1.0 * h * w / (n > 0 ? n : 1));
        int cnt = 0;
        for (;;) {
            if (cnt >= n) break;
            if (cnt > 0) {
                g -= 5;
                if (g < 7) { g = 7; break; }
            }
            if (g > kDsoMaxGridHost) {
                set_error("DSO grid %d exceeds the supported %d", g, kDsoMaxGridHost);
                return YGZFE_EINVAL;
            }
            const int ncells = (h / g) * (w / g);
            YGZ_TRY(ws.dso_keys.ensure((size_t)ncells * 3 * 4 + 16));
            YGZ_TRY(ws.dso_cnt.ensure((size_t)ncells * 4 + 16));
            YGZ_TRY(ws.dso_total.ensure(16));
            YGZ_HIP(launch_dso_pass(pyr, w, h, g, ws.occ.as<uint8_t>(), ws.dso_keys.as<uint32_t>(),
                                    ws.dso_cnt.as<int>(), st));
            YGZ_HIP(launch_dso_finish2(ws.dso_keys.as<uint32_t>(), ws.dso_cnt.as<int>(), ncells,
                                       ws.kps.as<ygzfe_kp>(), n_existing, ws.dso_total.as<int>(), st));
            YGZ_HIP(hipMemcpyAsync(&cnt, ws.dso_total.p, sizeof(int), hipMemcpyDeviceToHost, st));
            YGZ_HIP(hipStreamSynchronize(st));
            if (cnt == 0) break;  // the reference loops forever on a corner-free image
        }
        if (cnt > n) g += 5;
        ex->dso_grid = g;
        total = n_existing + cnt;
        YGZ_HIP(launch_desc_existing(pyr, ws.blur.as<uint8_t>(), pd.dp(), ws.kps.as<ygzfe_kp>(),
                                     ws.desc.as<uint8_t>(), total, 1, st));
        YGZ_HIP(hipStreamSynchronize(st));
    }
    *n_out = total;
    if (total > cap) {
        set_error("capacity %d < %d keypoints", cap, total);
        return YGZFE_ECAP;
    }
    if (total > 0) {
        YGZ_HIP(hipMemcpyAsync(kps_io, ws.kps.p, sizeof(ygzfe_kp) * total, hipMemcpyDeviceToHost, st));
        if (desc) YGZ_HIP(hipMemcpyAsync(desc, ws.desc.p, (size_t)32 * total, hipMemcpyDeviceToHost, st));
        YGZ_HIP(hipStreamSynchronize(st));
    }
    return YGZFE_OK;
}

int ygzfe_detect_and_compute(ygzfe_extractor *ex, ygzfe_frame *f, const uint8_t *img, int stride, ygzfe_kp *kps,
                             int cap, uint8_t *desc, int *n_out) {
    if (!img) { set_error("empty image"); return YGZFE_EINVAL; }  // reference returns silently (:972-973)
    YGZ_TRY(ygzfe_compute_pyramid(ex, f, img, stride));
    return ygzfe_extract(ex, f, YGZFE_ORBSLAM_KEYPOINT, kps, 0, cap, desc, n_out);
}

}  // extern "C"
