// api_align.cpp — the direct-method family: SparseImgAlign (single-frame and batch) with the
// align stream's placement probe, Align2D, the FAST-10 and DSO debug calls, direct projection
// and search, keyframe keypoints and the local-map set-up on the device.
#include <math.h>
#include <string.h>

#include <chrono>
#include <thread>

#include "host.hpp"

// Does work on `cand` run beside work on `stream`?  `stream` is held for 2 ms by
// one lane; an empty kernel on `cand` must finish inside the hold.  A stream that
// shares the hardware queue of `stream` waits for the hold instead.
int ygzfe_extractor::probe_beside(hipStream_t cand, bool &beside) {
    beside = false;
    YGZ_HIP(launch_empty(cand));  // the candidate's queue acquired, both streams idle
    YGZ_HIP(hipStreamSynchronize(cand));
    YGZ_HIP(hipStreamSynchronize(stream));
    hipEvent_t ea = nullptr, eb = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ea, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&eb, hipEventDisableTiming);
    if (e == hipSuccess) e = launch_hold_us(2000, stream);
    if (e == hipSuccess) e = hipEventRecord(ea, stream);
    if (e == hipSuccess) e = launch_empty(cand);
    if (e == hipSuccess) e = hipEventRecord(eb, cand);
    if (e == hipSuccess) {
        const auto t0 = std::chrono::steady_clock::now();
        while (hipEventQuery(eb) == hipErrorNotReady &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(50))
            std::this_thread::yield();
        beside = hipEventQuery(eb) == hipSuccess && hipEventQuery(ea) == hipErrorNotReady;
    }
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(cand);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (e != hipSuccess) { set_error("align stream probe: %s", hipGetErrorString(e)); return YGZFE_EHIP; }
    return YGZFE_OK;
}

int ygzfe_extractor::ensure_align_stream() {
    if (astream) return YGZFE_OK;
    // Normal priority, created on first use.  Measured alternatives (tools/run_lat_ab.sh):
    // the greatest / least priority, a dedicated queue (full CU mask) and creating the
    // extractor's streams eagerly all ran the single-frame path 15-30 % slower.
    // Streams beyond GPU_MAX_HW_QUEUES share hardware queues, and an align stream on the
    // extraction stream's queue runs after the extraction instead of beside it (0.28
    // instead of 0.16 ms per frame).  So each candidate is probed; a
    // rejected one stays alive until the choice is made (the next stream then lands on
    // another queue).  YGZFE_ALIGN_PROBE=0 keeps the first stream unprobed.
    YGZ_HIP(hipEventCreateWithFlags(&ev_align_fork, hipEventDisableTiming));
    YGZ_HIP(hipEventCreateWithFlags(&ev_align_done, hipEventDisableTiming));
    const char *pe = getenv("YGZFE_ALIGN_PROBE");
    const bool probe = !(pe && pe[0] == '0');
    std::vector<hipStream_t> rejected;
    int rc = YGZFE_OK;
    // at most 4 probes and 150 ms in all (another thread's work on the GPU can make
    // good candidates fail); then the next stream is taken unprobed
    const auto t_start = std::chrono::steady_clock::now();
    for (int attempt = 0; rc == YGZFE_OK && !astream; attempt++) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed");
            rc = YGZFE_EHIP;
            break;
        }
        bool beside = true;
        const bool in_budget = std::chrono::steady_clock::now() - t_start < std::chrono::milliseconds(150);
        const bool probed = probe && attempt < 4 && in_budget;
        if (probed) rc = probe_beside(s, beside);
        if (rc == YGZFE_OK && beside) {
            astream = s;
            align_probe_beside = probed ? 1 : 0;
        } else {
            rejected.push_back(s);
        }
        align_probe_attempts = attempt + 1;
    }
    for (hipStream_t s : rejected) (void)hipStreamDestroy(s);
    return rc;
}

// ------------------------------------------------------------------ sparse align
namespace ygzfe {
AlignLevels levels_of(const Plan &P) {
    AlignLevels lv;
    memset(&lv, 0, sizeof(lv));
    for (int l = 0; l < P.nlevels; l++) {
        lv.w[l] = P.lv[l].w;
        lv.h[l] = P.lv[l].h;
        lv.off[l] = P.lv[l].off;
        lv.inv_scale[l] = P.lv[l].inv_scale;
    }
    return lv;
}
}  // namespace ygzfe

extern "C" {

static int sparse_align_begin(const ygzfe_frame *ref, const ygzfe_frame *cur, const ygzfe_camera *cam,
                              const ygzfe_kp *kps, const float *xyz_ref, const uint8_t *usable, int n, int max_level,
                              int min_level, const ygzfe_se3 *T_init, int method) {
    if (method != YGZFE_ALIGN_GAUSS_NEWTON && method != YGZFE_ALIGN_LEVENBERG_MARQUARDT) {
        set_error("unknown SparseImgAlign method %d", method);
        return YGZFE_EINVAL;
    }
    if (!ref || !cur || !cam || !T_init || n < 0 || (n > 0 && (!kps || !xyz_ref || !usable))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (ref->plan != cur->plan) { set_error("ref and cur frames must share size and extractor"); return YGZFE_EINVAL; }
    const Plan &P = ref->plan->hp();
    if (min_level < 0 || max_level >= P.nlevels || min_level > max_level) {
        set_error("levels [%d,%d] outside the %d-level pyramid", min_level, max_level, P.nlevels);
        return YGZFE_EINVAL;
    }
    ygzfe_extractor *ex = ref->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    if (ex->align_pending) { set_error("a SparseImgAlign is already in flight on this extractor"); return YGZFE_ESTATE; }
    YGZ_TRY(ex->ensure_align_stream());
    YGZ_TRY(ex->ahout.ensure(sizeof(ygzfe_align_result)));
    if (n == 0) {  // SparseImageAlign.cc:24-27: no alignment, TCR untouched
        ygzfe_align_result *r = ex->ahout.as<ygzfe_align_result>();
        memset(r, 0, sizeof(*r));
        r->T_cur_ref = *T_init;
        r->chi2 = 1e10f;
        YGZ_HIP(hipEventRecord(ex->ev_align_done, ex->astream));
        ex->align_pending = true;
        return YGZFE_OK;
    }
    hipStream_t st = ex->astream;
    // after everything queued so far on the extractor stream (the two pyramids)
    YGZ_HIP(hipEventRecord(ex->ev_align_fork, ex->stream));
    YGZ_HIP(hipStreamWaitEvent(st, ex->ev_align_fork, 0));
    // A feature without a usable map point adds nothing to H, Jres, chi2 or the count
    // (SparseImageAlign.cc:67-75), so a reference frame with more keypoints than the
    // register kernel's threads (a keyframe after its DSO extraction, Frame.cc:717-771:
    // ~2,400 rows, only the tracked ones with map points) sends only its usable
    // features, in order, and stays on the register kernel
    const int n_all = n;
    int n_use = n;
    if (n > sparse_align_reg_capacity()) {
        n_use = 0;
        for (int i = 0; i < n; i++) n_use += usable[i] != 0;
    }
    n = n_use;
    // one packed H2D from pinned staging: [job][keypoints][xyz][usable] (16-B aligned
    // pieces), cached device buffers, one D2H of the result
    BlockLayout in{16};
    const size_t o_job = in.take(sizeof(AlignJob)), o_k = in.take(n, sizeof(ygzfe_kp)), o_x = in.take(n, 12);
    const size_t o_u = in.take(n), in_bytes = in.size(), spj = sparse_align_scratch_floats(n);
    YGZ_TRY(ex->align_in.ensure(in_bytes));
    YGZ_TRY(ex->align_scratch.ensure(sizeof(float) * spj));
    YGZ_TRY(ex->align_out.ensure(sizeof(ygzfe_align_result)));
    YGZ_TRY(ex->ahin.ensure(in_bytes));
    uint8_t *din = ex->align_in.as<uint8_t>(), *hin = ex->ahin.as<uint8_t>();
    AlignJob job;
    job.ref_pyr = ref->pyr.as<uint8_t>();
    job.cur_pyr = cur->pyr.as<uint8_t>();
    job.kps = at<const ygzfe_kp>(din, o_k);
    job.xyz = at<const float>(din, o_x);
    job.usable = din + o_u;
    job.n = n;
    job.max_level = max_level;
    job.min_level = min_level;
    job.method = method;
    job.T_init = *T_init;
    memcpy(hin + o_job, &job, sizeof(job));
    if (n == n_all) {
        memcpy(hin + o_k, kps, sizeof(ygzfe_kp) * (size_t)n);
        memcpy(hin + o_x, xyz_ref, sizeof(float) * 3 * (size_t)n);
        memcpy(hin + o_u, usable, (size_t)n);
    } else {
        ygzfe_kp *hk = at<ygzfe_kp>(hin, o_k);
        float *hx = at<float>(hin, o_x);
        for (int i = 0, j = 0; i < n_all; i++)
            if (usable[i]) {
                hk[j] = kps[i];
                memcpy(hx + 3 * (size_t)j, xyz_ref + 3 * (size_t)i, 3 * sizeof(float));
                j++;
            }
        memset(hin + o_u, 1, (size_t)n);
    }
    YGZ_HIP(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, st));
    YGZ_HIP(launch_sparse_align(levels_of(P), *cam, at<const AlignJob>(din, o_job), 1, ex->align_scratch.as<float>(),
                                spj, ex->align_out.as<ygzfe_align_result>(), st, n, method));
    YGZ_HIP(hipMemcpyAsync(ex->ahout.p, ex->align_out.p, sizeof(ygzfe_align_result), hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipEventRecord(ex->ev_align_done, st));
    ex->align_pending = true;
    return YGZFE_OK;
}

int ygzfe_extractor_align_probe(ygzfe_extractor *ex, int *attempts, int *passed) {
    if (!ex) { set_error("invalid argument"); return YGZFE_EINVAL; }
    std::lock_guard<std::mutex> lk(ex->mu);
    if (attempts) *attempts = ex->align_probe_attempts;
    if (passed) *passed = ex->align_probe_beside;
    return YGZFE_OK;
}

int ygzfe_sparse_align_end(const ygzfe_frame *cur, ygzfe_align_result *result) {
    if (!cur || !result) { set_error("invalid argument"); return YGZFE_EINVAL; }
    ygzfe_extractor *ex = cur->ex;
    std::lock_guard<std::mutex> lk(ex->mu);
    if (!ex->align_pending) { set_error("no SparseImgAlign in flight on this extractor"); return YGZFE_ESTATE; }
    YGZ_TRY(ensure_device(ex->device));
    ex->align_pending = false;
    YGZ_HIP(hipEventSynchronize(ex->ev_align_done));
    memcpy(result, ex->ahout.p, sizeof(*result));
    return YGZFE_OK;
}

int ygzfe_sparse_align_begin(const ygzfe_frame *ref, const ygzfe_frame *cur, const ygzfe_camera *cam,
                             const ygzfe_kp *kps, const float *xyz_ref, const uint8_t *usable, int n, int max_level,
                             int min_level, const ygzfe_se3 *T_init) {
    return sparse_align_begin(ref, cur, cam, kps, xyz_ref, usable, n, max_level, min_level, T_init,
                              YGZFE_ALIGN_GAUSS_NEWTON);
}

int ygzfe_sparse_align(const ygzfe_frame *ref, const ygzfe_frame *cur, const ygzfe_camera *cam, const ygzfe_kp *kps,
                       const float *xyz_ref, const uint8_t *usable, int n, int max_level, int min_level,
                       const ygzfe_se3 *T_init, ygzfe_align_result *result) {
    return ygzfe_sparse_align_method(ref, cur, cam, kps, xyz_ref, usable, n, max_level, min_level, T_init,
                                     YGZFE_ALIGN_GAUSS_NEWTON, result);
}

int ygzfe_sparse_align_method(const ygzfe_frame *ref, const ygzfe_frame *cur, const ygzfe_camera *cam,
                              const ygzfe_kp *kps, const float *xyz_ref, const uint8_t *usable, int n, int max_level,
                              int min_level, const ygzfe_se3 *T_init, int method, ygzfe_align_result *result) {
    if (!result) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(sparse_align_begin(ref, cur, cam, kps, xyz_ref, usable, n, max_level, min_level, T_init, method));
    return ygzfe_sparse_align_end(cur, result);
}

}  // extern "C"

extern "C" int ygzfe_batch_sparse_align(ygzfe_batch *b, int n_pairs, const int32_t *d_ref_idx,
                                        const int32_t *d_cur_idx, const float *d_xyz_ref, const uint8_t *d_usable,
                                        const ygzfe_camera *cam, int max_level, int min_level,
                                        const ygzfe_se3 *d_T_init, ygzfe_align_result *d_out, void *stream) {
    if (!b || !cam || n_pairs < 0 || !d_ref_idx || !d_cur_idx || !d_xyz_ref || !d_usable || !d_T_init || !d_out) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    const Plan &P = b->plan->hp();
    if (min_level < 0 || max_level >= P.nlevels || min_level > max_level) {
        set_error("levels [%d,%d] outside the %d-level pyramid", min_level, max_level, P.nlevels);
        return YGZFE_EINVAL;
    }
    if (n_pairs == 0) return YGZFE_OK;
    YGZ_TRY(ensure_device(b->device));
    hipStream_t st = stream ? (hipStream_t)stream : b->stream;
    const size_t spj = sparse_align_scratch_floats(P.kp_cap);
    YGZ_TRY(b->jobs.ensure(sizeof(AlignJob) * n_pairs));
    YGZ_TRY(b->ascratch.ensure(sizeof(float) * spj * n_pairs));
    YGZ_HIP(launch_build_align_jobs(b->jobs.as<AlignJob>(), n_pairs, d_ref_idx, d_cur_idx, b->pyr.as<uint8_t>(),
                                    P.pyr_bytes, b->ws.kps.as<ygzfe_kp>(), b->ws.counts.as<int32_t>(), P.kp_cap,
                                    d_xyz_ref, d_usable, max_level, min_level, d_T_init, st));
    hipEvent_t t0 = b->begin(st);
    YGZ_HIP(launch_sparse_align(levels_of(P), *cam, b->jobs.as<AlignJob>(), n_pairs, b->ascratch.as<float>(), spj,
                                d_out, st, P.kp_cap));
    b->end(ST_ALIGN, t0, st);
    return YGZFE_OK;
}

// ------------------------------------------------------------------ Align2D / direct projection
extern "C" int ygzfe_align2d_batch(const ygzfe_frame *cur, int level, int n, const uint8_t *patches_with_border,
                                   const uint8_t *patches, int n_iter, float *px_io, uint8_t *converged) {
    if (!cur || n < 0 || (n > 0 && (!patches_with_border || !patches || !px_io || !converged))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    const Plan &P = cur->plan->hp();
    if (level < 0 || level >= P.nlevels) { set_error("level out of range"); return YGZFE_EINVAL; }
    if (n == 0) return YGZFE_OK;
    ygzfe_extractor *ex = cur->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    hipStream_t st = ex->stream;
    BlockLayout in{16}, out{16};  // in: [patches with border][patches][px]  out: [px][converged]
    const size_t o_b = in.take(n, 100), o_p = in.take(n, 64), o_x = in.take(n, 8), in_bytes = in.size();
    const size_t o_px = out.take(n, 9), out_bytes = out.end();  // px and converged, packed
    YGZ_TRY(ex->direct_hin.ensure(in_bytes));
    YGZ_TRY(ex->direct_hout.ensure(out_bytes));
    YGZ_TRY(ex->direct_dev.ensure(in_bytes + out.size()));
    uint8_t *h = ex->direct_hin.as<uint8_t>(), *d = ex->direct_dev.as<uint8_t>();
    memcpy(h + o_b, patches_with_border, (size_t)n * 100);
    memcpy(h + o_p, patches, (size_t)n * 64);
    memcpy(h + o_x, px_io, (size_t)n * 8);
    YGZ_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    float *dpx = at<float>(d, in_bytes + o_px);
    uint8_t *dconv = d + in_bytes + o_px + (size_t)n * 8;
    YGZ_HIP(hipMemcpyAsync(dpx, d + o_x, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    const LevelDesc &L = P.lv[level];
    YGZ_HIP(launch_align2d(cur->pyr.as<uint8_t>() + L.off, L.w, L.h, n, d + o_b, d + o_p, n_iter, dpx, dconv, st));
    YGZ_HIP(hipMemcpyAsync(ex->direct_hout.p, dpx, out_bytes, hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipStreamSynchronize(st));
    memcpy(px_io, ex->direct_hout.p, (size_t)n * 8);
    memcpy(converged, ex->direct_hout.as<uint8_t>() + (size_t)n * 8, (size_t)n);
    return YGZFE_OK;
}

// FAST-10 (Thirdparty/fast) over host-image ROIs: the whole image and the ROI table
// go up in one DMA, one workgroup per ROI, the corner lists come back in one.
extern "C" int ygzfe_fast10_detect(int device, const uint8_t *img, int width, int height, int stride,
                                   const int32_t *rois, int n_roi, int barrier, int variant, int16_t *xy, int cap,
                                   int32_t *counts) {
    if (!img || width <= 0 || height <= 0 || stride < width || n_roi < 0 || (n_roi > 0 && (!rois || !counts)) ||
        cap < 0 || (cap > 0 && !xy) || (variant != 0 && variant != 1) || barrier < 0) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    for (int r = 0; r < n_roi; r++) {
        const int x0 = rois[4 * r], y0 = rois[4 * r + 1], w = rois[4 * r + 2], h = rois[4 * r + 3];
        if (w < 0 || h < 0) { set_error("roi %d: negative size", r); return YGZFE_EINVAL; }
        // the tested pixels (the whole ROI for the plain scan, its [3, -3) interior for SSE2
        // when w >= 22) with their radius-3 rings
        const int in = (variant == 1 && w >= 22) ? 3 : 0;
        if (w - 2 * in <= 0 || h - 2 * in <= 0) continue;
        if (x0 + in - 3 < 0 || y0 + in - 3 < 0 || x0 + w - in + 3 > width || y0 + h - in + 3 > height) {
            set_error("roi %d (%d, %d, %d, %d): the segment test would read outside the %dx%d image", r, x0, y0, w,
                      h, width, height);
            return YGZFE_EINVAL;
        }
    }
    if (n_roi == 0) return YGZFE_OK;
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    BlockLayout in{16}, out{16};  // in: [image][rois]  out: [counts][xy]
    const size_t o_img = in.take((size_t)stride * height), o_r = in.take(n_roi, 16), in_bytes = in.size();
    const size_t o_cnt = out.take(n_roi, 4), o_xy = out.take((size_t)n_roi * cap, 4), out_bytes = out.end();
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>();
    // the caller's last row may hold only `width` bytes (a cv::Mat ROI view)
    memcpy(h + o_img, img, (size_t)(height - 1) * stride + width);
    memcpy(h + o_r, rois, (size_t)n_roi * 16);
    YGZ_TRY(S.upload(in_bytes));
    YGZ_HIP(launch_fast10_rois(d + o_img, stride, at<const int>(d, o_r), n_roi, barrier, variant,
                               at<int16_t>(d, in_bytes + o_xy), cap, at<int32_t>(d, in_bytes + o_cnt), S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    memcpy(counts, S->hout.as<uint8_t>() + o_cnt, (size_t)n_roi * 4);
    if (cap > 0) memcpy(xy, S->hout.as<uint8_t>() + o_xy, (size_t)n_roi * cap * 4);
    for (int r = 0; r < n_roi; r++)
        if (counts[r] > cap) {
            set_error("roi %d: %d corners > cap %d", r, counts[r], cap);
            return YGZFE_ECAP;
        }
    return YGZFE_OK;
}

extern "C" int ygzfe_debug_dso_cells(int device, const uint8_t *img, int width, int height, int g, int barrier,
                                     uint8_t *flags) {
    if (!img || !flags || width <= 0 || height <= 0 || g < 7 || g > kDsoMaxGridHost) {
        set_error("invalid argument (g in [7, %d])", kDsoMaxGridHost);
        return YGZFE_EINVAL;
    }
    const size_t ncells = (size_t)(height / g) * (width / g), img_b = (size_t)width * height;
    BlockLayout blk{16};  // device block: [image][flags]
    const size_t fb = ncells * g * g, o_img = blk.take(img_b), o_f = blk.take(fb);
    if (ncells == 0) return YGZFE_OK;
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    YGZ_TRY(S->hin.ensure(img_b));  // not the lease's frame: the image goes up without its padding
    YGZ_TRY(S->hout.ensure(fb));
    YGZ_TRY(S->dev.ensure(blk.end()));
    uint8_t *d = S->dev.as<uint8_t>();
    memcpy(S->hin.p, img, img_b);
    YGZ_HIP(hipMemcpyAsync(d + o_img, S->hin.p, img_b, hipMemcpyHostToDevice, S->stream));
    YGZ_HIP(launch_dso_cells_debug(d + o_img, width, height, g, barrier, d + o_f, S->stream));
    YGZ_HIP(hipMemcpyAsync(S->hout.p, d + o_f, fb, hipMemcpyDeviceToHost, S->stream));
    YGZ_HIP(hipStreamSynchronize(S->stream));
    memcpy(flags, S->hout.p, fb);
    return YGZFE_OK;
}

// Align2D(const cv::Mat& cur_img, ...) on a host image: the 48 x 48 window around
// the estimate goes up (the whole image only when the iterations walk out of it).
extern "C" int ygzfe_align2d_image(int device, const uint8_t *img, int w, int h, int stride,
                                   const uint8_t *patch_with_border, const uint8_t *patch, int n_iter, float *px,
                                   uint8_t *converged) {
    if (!img || w <= 0 || h <= 0 || stride < w || !patch_with_border || !patch || !px || !converged) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    hipStream_t st = S->stream;
    // not the lease's frame: a fixed header and a 2-D window copy, no pinned staging
    const size_t small = 256;  // pwb 100 | p 64 | px 8 | status 4
    uint8_t host_small[small];
    memcpy(host_small, patch_with_border, 100);
    memcpy(host_small + 100, patch, 64);
    memcpy(host_small + 164, px, 8);
    const int half = 24;
    float fu = px[0], fv = px[1];
    int cu = std::isfinite(fu) ? (int)floorf(fu) : 0, cv = std::isfinite(fv) ? (int)floorf(fv) : 0;
    cu = std::min(std::max(cu, 0), w - 1);
    cv = std::min(std::max(cv, 0), h - 1);
    for (int pass = 0; pass < 2; pass++) {
        int x0 = 0, y0 = 0, ww = w, wh = h;
        if (pass == 0) {
            x0 = std::max(cu - half, 0);
            y0 = std::max(cv - half, 0);
            ww = std::min(cu + half, w) - x0;
            wh = std::min(cv + half, h) - y0;
        }
        YGZ_TRY(S->dev.ensure(small + (size_t)ww * wh));
        uint8_t *d = S->dev.as<uint8_t>();
        YGZ_HIP(hipMemcpyAsync(d, host_small, 172, hipMemcpyHostToDevice, st));
        YGZ_HIP(hipMemcpy2DAsync(d + small, ww, img + (size_t)y0 * stride + x0, stride, ww, wh,
                                 hipMemcpyHostToDevice, st));
        YGZ_HIP(launch_align2d_window(d + small, ww, w, h, x0, y0, ww, wh, d, d + 100, n_iter,
                                      reinterpret_cast<float *>(d + 164), reinterpret_cast<int *>(d + 172), st));
        uint8_t back[12];
        YGZ_HIP(hipMemcpyAsync(back, d + 164, 12, hipMemcpyDeviceToHost, st));
        YGZ_HIP(hipStreamSynchronize(st));
        int status;
        memcpy(&status, back + 8, 4);
        if (status >= 0) {
            memcpy(px, back, 8);
            *converged = (uint8_t)status;
            return YGZFE_OK;
        }
    }
    set_error("Align2D window retry failed");
    return YGZFE_EHIP;
}

extern "C" int ygzfe_find_direct_projection_batch(const ygzfe_frame *const *ref, const ygzfe_frame *cur,
                                                  const ygzfe_camera *cam, int n, const int32_t *ref_index,
                                                  const ygzfe_kp *kp_ref, const float *pt_ref, const ygzfe_se3 *T_cr,
                                                  float *px_io, int32_t *search_level, uint8_t *ok) {
    if (!ref || !cur || !cam || n < 0 ||
        (n > 0 && (!ref_index || !kp_ref || !pt_ref || !T_cr || !px_io || !search_level || !ok))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (n == 0) return YGZFE_OK;
    int nref = 0;
    for (int i = 0; i < n; i++) nref = std::max(nref, ref_index[i] + 1);
    for (int i = 0; i < n; i++)
        if (ref_index[i] < 0) { set_error("negative ref_index"); return YGZFE_EINVAL; }
    for (int r = 0; r < nref; r++)
        if (!ref[r] || ref[r]->plan != cur->plan) {
            set_error("reference keyframe %d missing or of a different size", r);
            return YGZFE_EINVAL;
        }
    ygzfe_extractor *ex = cur->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    hipStream_t st = ex->stream;
    const Plan &P = cur->plan->hp();
    BlockLayout in{16}, out{16};  // in: [ref ptrs][scale][ref_index][kps][pt][T]  out: [px][level][ok]
    const size_t o_ref = in.take(nref, sizeof(void *)), o_sc = in.take(P.nlevels, sizeof(float)), o_ri = in.take(n, 4);
    const size_t o_kp = in.take(n, sizeof(ygzfe_kp)), o_pt = in.take(n, 12), o_T = in.take(n, sizeof(ygzfe_se3));
    const size_t o_px = in.take(n, 8), in_bytes = in.size();
    const size_t o_out = out.take(n, 13), out_bytes = out.end();  // px, level and ok, packed
    YGZ_TRY(ex->direct_hin.ensure(in_bytes));
    YGZ_TRY(ex->direct_hout.ensure(out_bytes));
    YGZ_TRY(ex->direct_dev.ensure(in_bytes + out.size()));
    uint8_t *h = ex->direct_hin.as<uint8_t>(), *d = ex->direct_dev.as<uint8_t>();
    const uint8_t **ptrs = at<const uint8_t *>(h, o_ref);
    for (int r = 0; r < nref; r++) ptrs[r] = ref[r]->pyr.as<uint8_t>();
    float *sc = at<float>(h, o_sc);
    for (int l = 0; l < P.nlevels; l++) sc[l] = P.lv[l].scale;
    memcpy(h + o_ri, ref_index, 4 * (size_t)n);
    memcpy(h + o_kp, kp_ref, sizeof(ygzfe_kp) * n);
    memcpy(h + o_pt, pt_ref, 12 * (size_t)n);
    memcpy(h + o_T, T_cr, sizeof(ygzfe_se3) * n);
    memcpy(h + o_px, px_io, 8 * (size_t)n);
    YGZ_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    float *dpx = at<float>(d, in_bytes + o_out);
    int32_t *dlv = at<int32_t>(d, in_bytes + o_out + 8 * (size_t)n);
    uint8_t *dok = d + in_bytes + o_out + 12 * (size_t)n;
    YGZ_HIP(hipMemcpyAsync(dpx, d + o_px, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
    const AlignLevels lv = levels_of(P);
    YGZ_HIP(launch_find_direct(at<const uint8_t *const>(d, o_ref), lv, cur->pyr.as<uint8_t>(), lv, P.nlevels,
                               at<const float>(d, o_sc), ex->scales.inv_sigma2[1 < P.nlevels ? 1 : 0], *cam, n,
                               at<const int32_t>(d, o_ri), at<const ygzfe_kp>(d, o_kp), at<const float>(d, o_pt),
                               at<const ygzfe_se3>(d, o_T), dpx, dlv, dok, st));
    YGZ_HIP(hipMemcpyAsync(ex->direct_hout.p, dpx, out_bytes, hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipStreamSynchronize(st));
    const uint8_t *ho = ex->direct_hout.as<uint8_t>();
    memcpy(px_io, ho, 8 * (size_t)n);
    memcpy(search_level, ho + 8 * (size_t)n, 4 * (size_t)n);
    memcpy(ok, ho + 12 * (size_t)n, (size_t)n);
    return YGZFE_OK;
}

// SearchLocalPointsDirect (Tracking.cc:2258-2410): items of both phases in one
// packed H2D from pinned staging, k_direct_items + k_direct_replay, one packed D2H.
static int search_direct_impl(const ygzfe_frame *const *ref, int n_ref, const ygzfe_frame *cur,
                              const ygzfe_camera *cam, int n_cache, int n_local, const int32_t *item_ptr,
                              const int32_t *ref_index, const ygzfe_kp *kp_ref, const float *pt_ref,
                              const ygzfe_se3 *T_cr, const float *px_proj, float border, int grid_size,
                              int cache_hit_th, float *px_out, int32_t *matched_item, int32_t *status,
                              int *cache_success, int *local_ran) {
    const int n_points = n_cache + n_local;
    if (!ref || n_ref < 0 || !cur || !cam || n_cache < 0 || n_local < 0 ||
        (n_points > 0 && (!item_ptr || !px_proj || !px_out || !matched_item))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (grid_size <= 0) { set_error("grid_size must be positive"); return YGZFE_EINVAL; }
    const Plan &P = cur->plan->hp();
    const long ncell = (long)(P.lv[0].h / grid_size) * (P.lv[0].w / grid_size);
    if (ncell > kDirectMaxGridCells) {
        set_error("coverage grid of %ld cells exceeds %d", ncell, kDirectMaxGridCells);
        return YGZFE_EINVAL;
    }
    if (n_points == 0) {
        if (cache_success) *cache_success = 0;
        if (local_ran) *local_ran = !(0 > cache_hit_th);
        return YGZFE_OK;
    }
    if (item_ptr[0] != 0) { set_error("item_ptr[0] must be 0"); return YGZFE_EINVAL; }
    for (int i = 0; i < n_points; i++)
        if (item_ptr[i + 1] < item_ptr[i]) { set_error("item_ptr not monotone at %d", i); return YGZFE_EINVAL; }
    const int n_items = item_ptr[n_points];
    if (n_items > 0 && (!ref_index || !kp_ref || !pt_ref || !T_cr)) { set_error("null item array"); return YGZFE_EINVAL; }
    for (int k = 0; k < n_items; k++)
        if (ref_index[k] < 0 || ref_index[k] >= n_ref) { set_error("ref_index[%d] out of range", k); return YGZFE_EINVAL; }
    for (int k = 0; k < n_items; k++)
        if (kp_ref[k].octave < 0 || kp_ref[k].octave >= P.nlevels) {
            set_error("kp_ref[%d].octave %d out of range", k, kp_ref[k].octave);
            return YGZFE_EINVAL;
        }
    for (int r = 0; r < n_ref; r++)
        if (!ref[r] || ref[r]->plan != cur->plan) {
            set_error("reference keyframe %d missing or of a different size", r);
            return YGZFE_EINVAL;
        }
    ygzfe_extractor *ex = cur->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    hipStream_t st = ex->stream;
    // in: [ref ptrs][scale][item_ptr][px_proj][items][T table]   out: [hdr][px_out][matched][status] | [px_item][ok_item]
    // T table: one T_cr per keyframe slot while its items agree (Tracking's TCR is per
    // keyframe), else one per differing item
    std::vector<int32_t> slot_tcr((size_t)std::max(1, n_ref), -1);
    std::vector<ygzfe_se3> tab;
    tab.reserve(std::max(1, n_ref));
    BlockLayout in{256}, out{256};
    const size_t o_ptr = in.take(std::max(1, n_ref), sizeof(void *)), o_sc = in.take(kMaxLevels, 4);
    const size_t o_ip = in.take((size_t)n_points + 1, 4), o_pp = in.take(n_points, 8);
    const size_t o_it = in.take(n_items, sizeof(DirectItem));
    std::vector<int32_t> tcr_of((size_t)n_items);
    for (int k = 0; k < n_items; k++) {
        int &e = slot_tcr[ref_index[k]];
        if (e < 0 || memcmp(&tab[e], &T_cr[k], sizeof(ygzfe_se3)) != 0) {
            const int t = (int)tab.size();
            tab.push_back(T_cr[k]);
            if (e < 0) e = t;
            tcr_of[k] = t;
        } else {
            tcr_of[k] = e;
        }
    }
    const size_t o_tab = in.take(std::max<size_t>(1, tab.size()), sizeof(ygzfe_se3)), in_bytes = in.size();
    const size_t o_pxo = 16, o_m = o_pxo + 8 * (size_t)n_points, o_st = o_m + 4 * (size_t)n_points;
    const size_t o_hdr = out.take(o_st + 4 * (size_t)n_points), back_bytes = out.end();  // goes back, packed
    const size_t o_pxi = out.take(n_items, 8), o_ok = out.take(n_items), out_bytes = out.size();
    YGZ_TRY(ex->direct_hin.ensure(in_bytes));
    YGZ_TRY(ex->direct_hout.ensure(back_bytes));
    uint8_t *h = ex->direct_hin.as<uint8_t>();
    const uint8_t **ptrs = at<const uint8_t *>(h, o_ptr);
    for (int r = 0; r < n_ref; r++) ptrs[r] = ref[r]->pyr.as<uint8_t>();
    float *sc = at<float>(h, o_sc);
    for (int l = 0; l < P.nlevels; l++) sc[l] = P.lv[l].scale;
    memcpy(h + o_ip, item_ptr, 4 * ((size_t)n_points + 1));
    memcpy(h + o_pp, px_proj, 8 * (size_t)n_points);
    DirectItem *it = at<DirectItem>(h, o_it);
    for (int i = 0; i < n_points; i++)
        for (int k = item_ptr[i]; k < item_ptr[i + 1]; k++) {
            it[k].kp = kp_ref[k];
            memcpy(it[k].pt, pt_ref + 3 * (size_t)k, 12);
            it[k].ref = ref_index[k];
            it[k].point = i;
            it[k].tcr = tcr_of[k];
        }
    if (!tab.empty()) memcpy(h + o_tab, tab.data(), sizeof(ygzfe_se3) * tab.size());
    YGZ_TRY(ex->direct_dev.ensure(in_bytes + out_bytes));
    uint8_t *d = ex->direct_dev.as<uint8_t>(), *dout = d + in_bytes;
    YGZ_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    YGZ_HIP(launch_search_direct(at<const uint8_t *const>(d, o_ptr), levels_of(P), cur->pyr.as<uint8_t>(), P.nlevels,
                                 at<const float>(d, o_sc), ex->scales.inv_sigma2[1 < P.nlevels ? 1 : 0], *cam, n_cache,
                                 n_local, n_items, at<const int32_t>(d, o_ip), d + o_it, at<const ygzfe_se3>(d, o_tab),
                                 at<const float>(d, o_pp), at<float>(dout, o_pxi), dout + o_ok, border, grid_size,
                                 cache_hit_th, at<float>(dout, o_pxo), at<int32_t>(dout, o_m), at<int32_t>(dout, o_st),
                                 at<int32_t>(dout, o_hdr), st));
    uint8_t *hb = ex->direct_hout.as<uint8_t>();
    YGZ_HIP(hipMemcpyAsync(hb, dout, back_bytes, hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipStreamSynchronize(st));
    memcpy(px_out, hb + o_pxo, 8 * (size_t)n_points);
    memcpy(matched_item, hb + o_m, 4 * (size_t)n_points);
    if (status) memcpy(status, hb + o_st, 4 * (size_t)n_points);
    int32_t hdr[2];
    memcpy(hdr, hb + o_hdr, 8);
    if (cache_success) *cache_success = hdr[0];
    if (local_ran) *local_ran = hdr[1];
    return YGZFE_OK;
}

extern "C" int ygzfe_search_direct_batch(const ygzfe_frame *const *ref, int n_ref, const ygzfe_frame *cur,
                                         const ygzfe_camera *cam, int n_points, const int32_t *item_ptr,
                                         const int32_t *ref_index, const ygzfe_kp *kp_ref, const float *pt_ref,
                                         const ygzfe_se3 *T_cr, const float *px_proj, float border,
                                         float *px_out, int32_t *matched_item) {
    // the local-map loop alone (Tracking.cc:2348-2405): no grid, always runs
    return search_direct_impl(ref, n_ref, cur, cam, 0, n_points, item_ptr, ref_index, kp_ref, pt_ref, T_cr, px_proj,
                              border, 5, 0x7fffffff, px_out, matched_item, nullptr, nullptr, nullptr);
}

extern "C" int ygzfe_search_local_points_direct(const ygzfe_frame *const *ref, int n_ref, const ygzfe_frame *cur,
                                                const ygzfe_camera *cam, int n_cache, int n_local,
                                                const int32_t *item_ptr, const int32_t *ref_index,
                                                const ygzfe_kp *kp_ref, const float *pt_ref, const ygzfe_se3 *T_cr,
                                                const float *px_proj, float border, int grid_size, int cache_hit_th,
                                                float *px_out, int32_t *matched_item, int32_t *status,
                                                int *cache_success, int *local_ran) {
    return search_direct_impl(ref, n_ref, cur, cam, n_cache, n_local, item_ptr, ref_index, kp_ref, pt_ref, T_cr,
                              px_proj, border, grid_size, cache_hit_th, px_out, matched_item, status, cache_success,
                              local_ran);
}

// ------------------------------------------------------------------ local map, set up on the device
extern "C" int ygzfe_frame_set_keypoints(ygzfe_frame *f, const ygzfe_kp *kps, int n) {
    if (!f || n < 0 || (n > 0 && !kps)) { set_error("invalid argument"); return YGZFE_EINVAL; }
    const Plan &P = f->plan->hp();
    for (int i = 0; i < n; i++)
        if (kps[i].octave < 0 || kps[i].octave >= P.nlevels) {
            set_error("kps[%d].octave %d out of range", i, kps[i].octave);
            return YGZFE_EINVAL;
        }
    ygzfe_extractor *ex = f->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    YGZ_HIP(hipStreamSynchronize(ex->stream));  // no call in flight reads the old table
    YGZ_TRY(f->kps.ensure(sizeof(ygzfe_kp) * (size_t)std::max(1, n)));
    if (n > 0) {
        YGZ_HIP(hipMemcpyAsync(f->kps.p, kps, sizeof(ygzfe_kp) * (size_t)n, hipMemcpyHostToDevice, ex->stream));
        YGZ_HIP(hipStreamSynchronize(ex->stream));
    }
    f->n_kps = n;
    return YGZFE_OK;
}

extern "C" int ygzfe_frame_keypoint_count(const ygzfe_frame *f) { return f ? f->n_kps : -1; }

// One packed H2D (tables, candidates, observations), k_direct_setup + k_direct_scan_fill +
// the counted item search + k_direct_replay + k_direct_finish, one packed D2H: the call
// shape of search_direct_impl, with the item list built on the device.
extern "C" int ygzfe_search_local_map_direct(const ygzfe_frame *cur, const ygzfe_camera *cam,
                                             const ygzfe_direct_view *view, const ygzfe_direct_keyframes *kfs,
                                             const ygzfe_direct_candidates *cand, int n_sel, float border,
                                             int grid_size, int cache_hit_th, const ygzfe_direct_map_result *out,
                                             int *cache_success, int *local_ran) {
    if (!cur || !cam || !view || !kfs || !cand || !out || cand->n_cache < 0 || cand->n_local < 0 || kfs->n_kf < 0) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    const int n_kf = kfs->n_kf, n = cand->n_cache + cand->n_local;
    if (n_kf > 0 && (!kfs->ref || !kfs->kf_id || !kfs->kf_excluded || !kfs->T_rw || !kfs->T_cr)) {
        set_error("null keyframe table");
        return YGZFE_EINVAL;
    }
    if (n > 0 && (!cand->world || !cand->normal || !cand->min_dist || !cand->max_dist || !cand->skip || !cand->obs_ptr)) {
        set_error("null candidate array");
        return YGZFE_EINVAL;
    }
    if (n_sel < 1 || n_sel > YGZFE_DIRECT_MAX_SEL) {
        set_error("n_sel %d outside [1, %d]", n_sel, YGZFE_DIRECT_MAX_SEL);
        return YGZFE_EINVAL;
    }
    if (grid_size <= 0) { set_error("grid_size must be positive"); return YGZFE_EINVAL; }
    const Plan &P = cur->plan->hp();
    const long ncell = (long)(P.lv[0].h / grid_size) * (P.lv[0].w / grid_size);
    if (ncell > kDirectMaxGridCells) {
        set_error("coverage grid of %ld cells exceeds %d", ncell, kDirectMaxGridCells);
        return YGZFE_EINVAL;
    }
    if (n == 0) {
        if (cache_success) *cache_success = 0;
        if (local_ran) *local_ran = !(0 > cache_hit_th);
        return YGZFE_OK;
    }
    for (int k = 0; k < n_kf; k++)
        if (!kfs->ref[k] || kfs->ref[k]->ex != cur->ex || kfs->ref[k]->plan != cur->plan || kfs->ref[k]->n_kps < 0) {
            set_error("keyframe %d missing, of another extractor or size, or without keypoints", k);
            return YGZFE_EINVAL;
        }
    const int32_t *op = cand->obs_ptr;
    if (op[0] != 0) { set_error("obs_ptr[0] must be 0"); return YGZFE_EINVAL; }
    long max_items_l = 0;
    for (int i = 0; i < n; i++) {
        if (op[i + 1] < op[i]) { set_error("obs_ptr not monotone at %d", i); return YGZFE_EINVAL; }
        max_items_l += std::min(op[i + 1] - op[i], n_sel);
    }
    const int n_obs = op[n];
    if (n_obs > 0 && (!cand->obs_kf || !cand->obs_kp)) { set_error("null observation array"); return YGZFE_EINVAL; }
    for (int k = 0; k < n_obs; k++) {
        const int s = cand->obs_kf[k];
        if (s < 0 || s >= n_kf) { set_error("obs_kf[%d] out of range", k); return YGZFE_EINVAL; }
        if (cand->obs_kp[k] < 0 || cand->obs_kp[k] >= kfs->ref[s]->n_kps) {
            set_error("obs_kp[%d] = %d outside keyframe %d's %d keypoints", k, cand->obs_kp[k], s, kfs->ref[s]->n_kps);
            return YGZFE_EINVAL;
        }
    }
    if (max_items_l > 0x7fffffff / (long)sizeof(DirectItem)) { set_error("too many items"); return YGZFE_EINVAL; }
    const int max_items = (int)max_items_l;  // <= min(n_obs, n_sel * n)
    ygzfe_extractor *ex = cur->ex;
    YGZ_TRY(ensure_device(ex->device));
    std::lock_guard<std::mutex> lk(ex->mu);
    hipStream_t st = ex->stream;
    BlockLayout li{256}, lo{256};
    const size_t nk = (size_t)std::max(1, n_kf), N = (size_t)n;
    // in: [ref ptrs][kp ptrs][scale][kf_id][T_rw][T_cr][excluded] [world][normal][min][max][obs_ptr][skip] [obs_kf][obs_kp]
    const size_t i_ref = li.take(nk, 8), i_kpp = li.take(nk, 8), i_sc = li.take(kMaxLevels, 4), i_id = li.take(nk, 8);
    const size_t i_trw = li.take(nk, 48), i_tcr = li.take(nk, sizeof(ygzfe_se3)), i_ex = li.take(nk);
    const size_t i_w = li.take(N, 12), i_nr = li.take(N, 12), i_mn = li.take(N, 4), i_mx = li.take(N, 4);
    const size_t i_op = li.take(N + 1, 4), i_sk = li.take(N), i_ok = li.take(n_obs, 4), i_oq = li.take(n_obs, 4);
    // back, packed: [hdr][status][px_out][matched_kf][matched_kp][proj][view_cos][dist]
    const size_t b_st = 16, b_px = b_st + 4 * N, b_mk = b_px + 8 * N, b_mp = b_mk + 4 * N, b_pj = b_mp + 4 * N;
    const size_t b_vc = b_pj + 12 * N, b_ds = b_vc + 4 * N, b_hdr = lo.take(b_ds + 4 * N), back_bytes = lo.end();
    // scratch: [culled][cnt][bsum][sel_kf][sel_kp][item_ptr][n_items][px_proj][matched_item][items][px_item][ok_item]
    const size_t nblk = (N + kDirectSetupThreads - 1) / kDirectSetupThreads, M = (size_t)max_items;
    const size_t nsel = kDirectMaxSel * N, s_cu = lo.take(N), s_cn = lo.take(N, 4), s_bs = lo.take(nblk, 4);
    const size_t s_sf = lo.take(nsel, 4), s_sp = lo.take(nsel, 4), s_ip = lo.take(N + 1, 4), s_ni = lo.take(4);
    const size_t s_pp = lo.take(N, 8), s_mi = lo.take(N, 4), s_it = lo.take(M, sizeof(DirectItem));
    const size_t s_pi = lo.take(M, 8), s_oi = lo.take(M), in_bytes = li.size(), out_bytes = lo.size();
    YGZ_TRY(ex->direct_hin.ensure(in_bytes));
    YGZ_TRY(ex->direct_hout.ensure(back_bytes));
    YGZ_TRY(ex->direct_dev.ensure(in_bytes + out_bytes));
    uint8_t *h = ex->direct_hin.as<uint8_t>(), *d = ex->direct_dev.as<uint8_t>(), *dout = d + in_bytes;
    const uint8_t **ptrs = at<const uint8_t *>(h, i_ref);
    const ygzfe_kp **kpp = at<const ygzfe_kp *>(h, i_kpp);
    for (int k = 0; k < n_kf; k++) {
        ptrs[k] = kfs->ref[k]->pyr.as<uint8_t>();
        kpp[k] = kfs->ref[k]->kps.as<ygzfe_kp>();
    }
    float *sc = at<float>(h, i_sc);
    for (int l = 0; l < P.nlevels; l++) sc[l] = P.lv[l].scale;
    if (n_kf > 0) {
        memcpy(h + i_id, kfs->kf_id, 8 * (size_t)n_kf);
        memcpy(h + i_trw, kfs->T_rw, 48 * (size_t)n_kf);
        memcpy(h + i_tcr, kfs->T_cr, sizeof(ygzfe_se3) * (size_t)n_kf);
        memcpy(h + i_ex, kfs->kf_excluded, (size_t)n_kf);
    }
    memcpy(h + i_w, cand->world, 12 * N);
    memcpy(h + i_nr, cand->normal, 12 * N);
    memcpy(h + i_mn, cand->min_dist, 4 * N);
    memcpy(h + i_mx, cand->max_dist, 4 * N);
    memcpy(h + i_op, op, 4 * (N + 1));
    memcpy(h + i_sk, cand->skip, N);
    if (n_obs > 0) {
        memcpy(h + i_ok, cand->obs_kf, 4 * (size_t)n_obs);
        memcpy(h + i_oq, cand->obs_kp, 4 * (size_t)n_obs);
    }
    YGZ_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    DirectMapDev in;
    in.world = at<const float>(d, i_w);
    in.normal = at<const float>(d, i_nr);
    in.min_dist = at<const float>(d, i_mn);
    in.max_dist = at<const float>(d, i_mx);
    in.skip = d + i_sk;
    in.obs_ptr = at<const int32_t>(d, i_op);
    in.obs_kf = at<const int32_t>(d, i_ok);
    in.obs_kp = at<const int32_t>(d, i_oq);
    in.kf_id = at<const int64_t>(d, i_id);
    in.kf_excluded = d + i_ex;
    in.T_rw = at<const float>(d, i_trw);
    in.kf_kps = at<const ygzfe_kp *const>(d, i_kpp);
    DirectMapWork w;
    w.culled = dout + s_cu;
    w.cnt = at<int32_t>(dout, s_cn);
    w.bsum = at<int32_t>(dout, s_bs);
    w.sel_kf = at<int32_t>(dout, s_sf);
    w.sel_kp = at<int32_t>(dout, s_sp);
    w.item_ptr = at<int32_t>(dout, s_ip);
    w.n_items = at<int32_t>(dout, s_ni);
    w.items = dout + s_it;
    w.px_proj = at<float>(dout, s_pp);
    w.px_item = at<float>(dout, s_pi);
    w.ok_item = dout + s_oi;
    w.matched_item = at<int32_t>(dout, s_mi);
    w.hdr = at<int32_t>(dout, b_hdr);
    w.status = at<int32_t>(dout, b_st);
    w.px_out = at<float>(dout, b_px);
    w.matched_kf = at<int32_t>(dout, b_mk);
    w.matched_kp = at<int32_t>(dout, b_mp);
    w.proj = at<float>(dout, b_pj);
    w.view_cos = at<float>(dout, b_vc);
    w.dist = at<float>(dout, b_ds);
    YGZ_HIP(launch_search_local_map(at<const uint8_t *const>(d, i_ref), levels_of(P), cur->pyr.as<uint8_t>(), P.nlevels,
                                    at<const float>(d, i_sc), ex->scales.inv_sigma2[1 < P.nlevels ? 1 : 0], *cam, *view,
                                    cand->n_cache, cand->n_local, n_sel, max_items, in, at<const ygzfe_se3>(d, i_tcr),
                                    w, border, grid_size, cache_hit_th, st));
    uint8_t *hb = ex->direct_hout.as<uint8_t>();
    YGZ_HIP(hipMemcpyAsync(hb, dout, back_bytes, hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipStreamSynchronize(st));
    if (out->status) memcpy(out->status, hb + b_st, 4 * N);
    if (out->px_out) memcpy(out->px_out, hb + b_px, 8 * N);
    if (out->matched_kf) memcpy(out->matched_kf, hb + b_mk, 4 * N);
    if (out->matched_kp) memcpy(out->matched_kp, hb + b_mp, 4 * N);
    if (out->proj) memcpy(out->proj, hb + b_pj, 12 * N);
    if (out->view_cos) memcpy(out->view_cos, hb + b_vc, 4 * N);
    if (out->dist) memcpy(out->dist, hb + b_ds, 4 * N);
    int32_t hdr[2];
    memcpy(hdr, hb + b_hdr, 8);
    if (cache_success) *cache_success = hdr[0];
    if (local_ran) *local_ran = hdr[1];
    return YGZFE_OK;
}
