// api_match.cpp — the match-frame handle and the ORBmatcher searches over it.
#include <string.h>

#include <cmath>
#include "host.hpp"

// --------------------------------------------------------------------------
// ORBmatcher searches (match.hip): the searched frame's state on the device,
// one packed H2D of the queries, two launches, one packed D2H of the results.
struct ygzfe_match_frame {
    int device = 0;
    hipStream_t stream = nullptr;
    int n = 0;
    bool has_uright = false;
    ygzfe_bounds bounds{0.f, 0.f, 0.f, 0.f};
    float inv_w = 0.f, inv_h = 0.f;
    DevBuf kps, desc, uright, cell;
    std::vector<ygzfe_kp> host_kps;  // angles / octaves / positions the host-side query building reads
    int last_rescans = 0;            // queries of the last search whose top-K list the skips exhausted
    int last_passes = -1;            // parallel-resolve passes of the last search (-1: serial replay)
    // per-call staging: page-locked, one DMA per direction; ev_in = the last H2D out of
    // hin / hset (the next call refills them only after it)
    DevBuf in, out, scratch;
    HostBuf hin, hout, hset;
    hipEvent_t ev_in = nullptr, ev_set = nullptr;
    // recorded on `stream` once the frame's keypoints, descriptors and grid are on the
    // device: a search on another frame's stream that reads this frame's descriptors as
    // its queries (SearchForInitialization, SearchByBoW) waits for it
    hipEvent_t ev_ready = nullptr;
};

namespace {

constexpr int kMatchTopK = 32;  // match.hip kTopList (J.topk stride)
constexpr int kMatchCells = 64 * 48;  // FRAME_GRID_COLS x ROWS

int match_frame_finish(ygzfe_match_frame *f, const ygzfe_bounds *bounds) {
    f->bounds = *bounds;
    // Frame.cc:296-297
    f->inv_w = (float)64 / (float)(bounds->max_x - bounds->min_x);
    f->inv_h = (float)48 / (float)(bounds->max_y - bounds->min_y);
    // cell[n] | cell ends [64 * 48] | keypoints by cell u16[n]
    YGZ_TRY(f->cell.ensure(sizeof(int32_t) * ((size_t)f->n + kMatchCells) + sizeof(uint16_t) * (size_t)f->n + 16));
    YGZ_HIP(launch_match_cells(f->kps.as<ygzfe_kp>(), f->n, bounds->min_x, bounds->min_y, f->inv_w, f->inv_h,
                               f->cell.as<int32_t>(), f->cell.as<int32_t>() + f->n,
                               reinterpret_cast<uint16_t *>(f->cell.as<int32_t>() + f->n + kMatchCells), f->stream));
    // no host synchronisation: a search on this frame runs on f->stream after the grid;
    // one that reads this frame's descriptors from another stream waits on ev_ready
    if (!f->ev_ready) YGZ_HIP(hipEventCreateWithFlags(&f->ev_ready, hipEventDisableTiming));
    YGZ_HIP(hipEventRecord(f->ev_ready, f->stream));
    return YGZFE_OK;
}

// Run one search problem: the job's host-side arrays are staged into one H2D
// copy; outputs come back in one D2H copy.
struct MatchCall {
    ygzfe_match_frame *train;
    std::vector<ygzfe_match_query> q;
    const uint8_t *qdesc_host = nullptr;  // [n_qdesc][32] (host) or
    const uint8_t *qdesc_dev = nullptr;   // device descriptors (INIT / BoW: a match frame's)
    const ygzfe_match_frame *qframe = nullptr;  // the match frame that owns qdesc_dev
    int n_qdesc = 0;
    std::vector<int32_t> qid, cand_ptr;
    const int32_t *cand_host = nullptr;
    int n_cand = 0;
    const uint8_t *blocked_host = nullptr;
    int mode = 0, th_dist = 100, check_ori = 0;
    float nnratio = 0.6f;
    // outputs
    int32_t *train_out = nullptr, *query_out = nullptr;
    int nmatches = 0;
};

int run_match(MatchCall &c) {
    ygzfe_match_frame *f = c.train;
    const int nq = (int)c.q.size(), n = f->n;
    if (n > 65535) { set_error("match frame holds %d keypoints (<= 65535 supported)", n); return YGZFE_EINVAL; }
    if (c.mode == YGZFE_MATCH_INIT && (n > 16384 || nq > 32767)) {
        set_error("SearchForInitialization: %d x %d keypoints exceed 32767 x 16384", nq, n);
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(f->device));
    hipStream_t st = f->stream;
    // query descriptors of another match frame: uploaded on that frame's stream
    if (c.qframe && c.qframe != f && c.qframe->ev_ready) YGZ_HIP(hipStreamWaitEvent(st, c.qframe->ev_ready, 0));
    // device input layout
    BlockLayout ai{256}, ao{256};
    const size_t o_q = ai.take(std::max(nq, 1), sizeof(ygzfe_match_query));
    const size_t o_qd = c.qdesc_host ? ai.take(std::max(c.n_qdesc, 1), 32) : 0;
    const size_t o_qid = c.qid.empty() ? 0 : ai.take(c.qid.size(), sizeof(int32_t));
    const size_t o_cp = c.cand_ptr.empty() ? 0 : ai.take(c.cand_ptr.size(), sizeof(int32_t));
    const size_t o_c = c.cand_host ? ai.take(std::max(c.n_cand, 1), sizeof(int32_t)) : 0;
    const size_t o_bl = c.blocked_host ? ai.take(std::max(n, 1)) : 0;
    // device outputs / scratch
    const size_t o_tout = ao.take(std::max(n, 1), sizeof(int32_t));
    const size_t o_qout = ao.take(std::max(nq, 1), sizeof(int32_t));
    const size_t o_nm = ao.take(4, sizeof(int32_t));
    const size_t out_bytes = ao.size();  // what comes back; the scratch parts follow
    const size_t o_topk = ao.take((size_t)kMatchTopK * std::max(nq, 1), sizeof(uint64_t));
    const size_t o_ncand = ao.take(std::max(nq, 1), sizeof(int32_t));
    const size_t o_push = ao.take(std::max(nq, 1), sizeof(int32_t));
    const size_t o_qang = ao.take(std::max(nq, 1), sizeof(float));
    YGZ_TRY(f->out.ensure(ao.size()));
    uint8_t *dout = f->out.as<uint8_t>();
    // The inputs stay in page-locked host memory that the kernels read directly (one
    // pass in k_match_topk, which copies what the decisions need into HBM): no H2D
    // copy and no copy-to-kernel dependency on the stream.  The previous call
    // synchronised its stream, so the staging is free.
    YGZ_TRY(f->hin.ensure(ai.size()));
    uint8_t *h = f->hin.as<uint8_t>(), *din = nullptr;
    YGZ_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&din), h, 0));
    MatchJob J;
    memset(&J, 0, sizeof(J));
    J.kps = f->kps.as<ygzfe_kp>();
    J.desc = f->desc.as<uint8_t>();
    J.u_right = f->has_uright ? f->uright.as<float>() : nullptr;
    J.cell = f->cell.as<int32_t>();
    J.cend = J.cell + n;
    J.cidx = reinterpret_cast<const uint16_t *>(J.cend + kMatchCells);
    J.n_train = n;
    J.min_x = f->bounds.min_x;
    J.min_y = f->bounds.min_y;
    J.inv_w = f->inv_w;
    J.inv_h = f->inv_h;
    J.q = at<const ygzfe_match_query>(din, o_q);
    J.qdesc = c.qdesc_host ? din + o_qd : c.qdesc_dev;
    J.qid = c.qid.empty() ? nullptr : at<const int32_t>(din, o_qid);
    J.nq = nq;
    J.cand_ptr = c.cand_ptr.empty() ? nullptr : at<const int32_t>(din, o_cp);
    J.cand = c.cand_host ? at<const int32_t>(din, o_c) : nullptr;
    J.blocked0 = c.blocked_host ? din + o_bl : nullptr;
    J.topk = at<uint64_t>(dout, o_topk);
    J.ncand = at<int32_t>(dout, o_ncand);
    J.qangle = at<float>(dout, o_qang);
    J.train_out = at<int32_t>(dout, o_tout);
    J.query_out = at<int32_t>(dout, o_qout);
    J.pushes = at<int32_t>(dout, o_push);
    J.nmatches = at<int32_t>(dout, o_nm);
    if (nq) memcpy(h + o_q, c.q.data(), sizeof(ygzfe_match_query) * nq);
    if (c.qdesc_host && c.n_qdesc) memcpy(h + o_qd, c.qdesc_host, (size_t)32 * c.n_qdesc);
    if (!c.qid.empty()) memcpy(h + o_qid, c.qid.data(), sizeof(int32_t) * c.qid.size());
    if (!c.cand_ptr.empty()) memcpy(h + o_cp, c.cand_ptr.data(), sizeof(int32_t) * c.cand_ptr.size());
    if (c.cand_host && c.n_cand) memcpy(h + o_c, c.cand_host, sizeof(int32_t) * c.n_cand);
    if (c.blocked_host && n) memcpy(h + o_bl, c.blocked_host, (size_t)n);
    // YGZFE_MATCH_PASSES=0 selects the serial replay (tests run both paths)
    const char *ev = getenv("YGZFE_MATCH_PASSES");
    const int max_passes = ev ? atoi(ev) : 1;
    YGZ_TRY(f->hout.ensure(out_bytes));
    const bool direct = match_resolves(n, nq, c.mode, max_passes);
    if (direct) {  // k_match_resolve writes each output once, straight into page-locked host memory
        uint8_t *hod = nullptr;
        YGZ_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&hod), f->hout.p, 0));
        J.train_out = at<int32_t>(hod, o_tout);
        J.nmatches = at<int32_t>(hod, o_nm);
    }
    YGZ_HIP(launch_match(J, c.mode, c.th_dist, c.check_ori, c.nnratio, max_passes, st));
    if (!direct) YGZ_HIP(hipMemcpyAsync(f->hout.p, dout, out_bytes, hipMemcpyDeviceToHost, st));
    YGZ_HIP(hipStreamSynchronize(st));
    const uint8_t *ho = f->hout.as<uint8_t>();
    if (c.train_out && n) memcpy(c.train_out, ho + o_tout, sizeof(int32_t) * n);
    if (c.query_out && nq) memcpy(c.query_out, ho + o_qout, sizeof(int32_t) * nq);
    memcpy(&c.nmatches, ho + o_nm, sizeof(int32_t));
    memcpy(&f->last_rescans, ho + o_nm + 4, sizeof(int32_t));
    memcpy(&f->last_passes, ho + o_nm + 8, sizeof(int32_t));
    if (max_passes > 0 && f->last_passes < 0 && c.mode != YGZFE_MATCH_INIT && nq > 0 && nq <= 4096 &&
        resolve_fits(n, nq)) {
        set_error("match resolve did not reach its fixed point within nq + 2 passes (internal error)");
        return YGZFE_EHIP;
    }
    return YGZFE_OK;
}

}  // namespace

extern "C" int ygzfe_match_frame_create(int device, ygzfe_match_frame **out) {
    if (!out) { set_error("null out"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(device));
    std::unique_ptr<ygzfe_match_frame> f(new ygzfe_match_frame());
    f->device = device;
    YGZ_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    *out = f.release();
    return YGZFE_OK;
}

extern "C" void ygzfe_match_frame_destroy(ygzfe_match_frame *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream), (void)hipStreamDestroy(f->stream);
    if (f->ev_in) (void)hipEventDestroy(f->ev_in);
    if (f->ev_set) (void)hipEventDestroy(f->ev_set);
    if (f->ev_ready) (void)hipEventDestroy(f->ev_ready);
    delete f;
}

extern "C" int ygzfe_match_frame_stats(const ygzfe_match_frame *f, int *rescans) {
    if (!f || !rescans) { set_error("invalid argument"); return YGZFE_EINVAL; }
    *rescans = f->last_rescans;
    return YGZFE_OK;
}

extern "C" int ygzfe_match_frame_resolve_stats(const ygzfe_match_frame *f, int *passes) {
    if (!f || !passes) { set_error("invalid argument"); return YGZFE_EINVAL; }
    *passes = f->last_passes;
    return YGZFE_OK;
}

extern "C" int ygzfe_match_frame_set(ygzfe_match_frame *f, const ygzfe_kp *kps, const uint8_t *desc, int n,
                                     const float *u_right, const ygzfe_bounds *bounds) {
    if (!f || !bounds || n < 0 || n > 65535 || (n > 0 && (!kps || !desc))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (!(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y)) {
        set_error("empty image bounds");
        return YGZFE_EINVAL;
    }
    YGZ_TRY(ensure_device(f->device));
    f->n = n;
    f->host_kps.assign(kps, kps + n);
    YGZ_TRY(f->kps.ensure(sizeof(ygzfe_kp) * (size_t)std::max(n, 1)));
    YGZ_TRY(f->desc.ensure((size_t)32 * std::max(n, 1)));
    f->has_uright = u_right != nullptr;
    if (u_right) YGZ_TRY(f->uright.ensure(sizeof(float) * (size_t)std::max(n, 1)));
    if (n) {  // keypoints, descriptors (and u_right) through page-locked staging: async DMAs
        const size_t kb = sizeof(ygzfe_kp) * (size_t)n, db = (size_t)32 * n, ub = u_right ? sizeof(float) * n : 0;
        if (f->ev_set) YGZ_HIP(hipEventSynchronize(f->ev_set));  // the previous frame's DMA out of hset
        // test hook (tests/test_gpu_match_search.py): hold this frame's stream before its
        // upload, so a search on another frame's stream that skipped the ev_ready wait
        // would read descriptors that are not there yet
        if (const char *hold = getenv("YGZFE_DEBUG_SET_HOLD_US")) YGZ_HIP(launch_hold_us(atoi(hold), f->stream));
        YGZ_TRY(f->hset.ensure(kb + db + ub));
        uint8_t *hs = f->hset.as<uint8_t>();
        memcpy(hs, kps, kb);
        memcpy(hs + kb, desc, db);
        if (ub) memcpy(hs + kb + db, u_right, ub);
        YGZ_HIP(hipMemcpyAsync(f->kps.p, hs, kb, hipMemcpyHostToDevice, f->stream));
        YGZ_HIP(hipMemcpyAsync(f->desc.p, hs + kb, db, hipMemcpyHostToDevice, f->stream));
        if (ub) YGZ_HIP(hipMemcpyAsync(f->uright.p, hs + kb + db, ub, hipMemcpyHostToDevice, f->stream));
        if (!f->ev_set) YGZ_HIP(hipEventCreateWithFlags(&f->ev_set, hipEventDisableTiming));
        YGZ_HIP(hipEventRecord(f->ev_set, f->stream));
    }
    return match_frame_finish(f, bounds);
}

extern "C" int ygzfe_match_frame_from_batch(ygzfe_match_frame *f, ygzfe_batch *b, int frame,
                                            const ygzfe_bounds *bounds) {
    if (!f || !b || !bounds || frame < 0 || frame >= b->maxF) { set_error("invalid argument"); return YGZFE_EINVAL; }
    if (f->device != b->device) { set_error("match frame and batch on different devices"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(f->device));
    const Plan &P = b->plan->hp();
    YGZ_TRY(batch_wait(b));  // the batch's extraction may run on caller streams
    int n = 0;
    YGZ_HIP(hipMemcpy(&n, b->ws.counts.as<int>() + frame, sizeof(int), hipMemcpyDeviceToHost));
    f->n = n;
    YGZ_TRY(f->kps.ensure(sizeof(ygzfe_kp) * (size_t)std::max(n, 1)));
    YGZ_TRY(f->desc.ensure((size_t)32 * std::max(n, 1)));
    f->host_kps.resize(n);
    if (n) {
        YGZ_HIP(hipMemcpyAsync(f->kps.p, b->ws.kps.as<ygzfe_kp>() + (size_t)frame * P.kp_cap, sizeof(ygzfe_kp) * n,
                               hipMemcpyDeviceToDevice, f->stream));
        YGZ_HIP(hipMemcpyAsync(f->desc.p, b->ws.desc.as<uint8_t>() + (size_t)frame * P.kp_cap * 32, (size_t)32 * n,
                               hipMemcpyDeviceToDevice, f->stream));
        YGZ_HIP(hipMemcpyAsync(f->host_kps.data(), f->kps.p, sizeof(ygzfe_kp) * n, hipMemcpyDeviceToHost, f->stream));
    }
    f->has_uright = false;
    YGZ_TRY(match_frame_finish(f, bounds));
    // host_kps (read by the host when this frame is a SearchForInitialization / BoW query
    // frame) arrives by the async D2H above
    YGZ_HIP(hipStreamSynchronize(f->stream));
    return YGZFE_OK;
}

extern "C" int ygzfe_search_projection_best(ygzfe_match_frame *cur, const ygzfe_match_query *q, const uint8_t *q_desc,
                                            int nq, const uint8_t *train_blocked, int th_dist, int check_ori,
                                            int32_t *train_match, int *nmatches) {
    if (!cur || nq < 0 || (nq > 0 && (!q || !q_desc)) || !train_match || !nmatches) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    MatchCall c;
    c.train = cur;
    c.q.assign(q, q + nq);
    c.qdesc_host = q_desc;
    c.n_qdesc = nq;
    c.blocked_host = train_blocked;
    c.mode = YGZFE_MATCH_BEST;
    c.th_dist = th_dist;
    c.check_ori = check_ori;
    c.train_out = train_match;
    YGZ_TRY(run_match(c));
    *nmatches = c.nmatches;
    return YGZFE_OK;
}

extern "C" int ygzfe_search_projection_ratio(ygzfe_match_frame *F, const ygzfe_match_query *q, const uint8_t *q_desc,
                                             int nq, const uint8_t *train_blocked, float nnratio, int32_t *train_match,
                                             int *nmatches) {
    if (!F || nq < 0 || (nq > 0 && (!q || !q_desc)) || !train_match || !nmatches) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    MatchCall c;
    c.train = F;
    c.q.assign(q, q + nq);
    c.qdesc_host = q_desc;
    c.n_qdesc = nq;
    c.blocked_host = train_blocked;
    c.mode = YGZFE_MATCH_RATIO;
    c.nnratio = nnratio;
    c.train_out = train_match;
    YGZ_TRY(run_match(c));
    *nmatches = c.nmatches;
    return YGZFE_OK;
}

extern "C" int ygzfe_search_for_initialization(ygzfe_match_frame *F1, ygzfe_match_frame *F2, float *prev_matched,
                                               int window_size, float nnratio, int check_ori, int32_t *matches12,
                                               int *nmatches) {
    if (!F1 || !F2 || (F1->n > 0 && (!prev_matched || !matches12)) || !nmatches) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (F1->device != F2->device) { set_error("frames on different devices"); return YGZFE_EINVAL; }
    // ORBmatcher.cc:388-398: queries = F1's keypoints, level-0 only, window at vbPrevMatched
    MatchCall c;
    c.train = F2;
    c.q.resize(F1->n);
    for (int i = 0; i < F1->n; i++) {
        ygzfe_match_query &Q = c.q[i];
        const ygzfe_kp &kp = F1->host_kps[i];
        Q.u = prev_matched[2 * i];
        Q.v = prev_matched[2 * i + 1];
        Q.radius = (float)window_size;
        Q.u_right = 0.f;
        Q.min_level = kp.octave;
        Q.max_level = kp.octave;
        Q.angle = kp.angle;
        Q.flags = kp.octave > 0 ? 0 : YGZFE_MQ_VALID;
    }
    c.qdesc_dev = F1->desc.as<uint8_t>();
    c.qframe = F1;
    c.mode = YGZFE_MATCH_INIT;
    c.nnratio = nnratio;
    c.check_ori = check_ori;
    c.query_out = matches12;
    YGZ_TRY(run_match(c));
    *nmatches = c.nmatches;
    // :472-475 update prev matched
    for (int i = 0; i < F1->n; i++)
        if (matches12[i] >= 0) {
            prev_matched[2 * i] = F2->host_kps[matches12[i]].x;
            prev_matched[2 * i + 1] = F2->host_kps[matches12[i]].y;
        }
    return YGZFE_OK;
}

extern "C" int ygzfe_search_by_bow(ygzfe_match_frame *kf, ygzfe_match_frame *F, const uint8_t *kf_usable,
                                   int n_kf_nodes, const int32_t *kf_nodes, const int32_t *kf_ptr,
                                   const int32_t *kf_feats, int n_f_nodes, const int32_t *f_nodes,
                                   const int32_t *f_ptr, const int32_t *f_feats, float nnratio, int check_ori,
                                   int32_t *f_match, int *nmatches) {
    if (!kf || !F || !kf_usable || !f_match || !nmatches || n_kf_nodes < 0 || n_f_nodes < 0 ||
        (n_kf_nodes > 0 && (!kf_nodes || !kf_ptr || !kf_feats)) || (n_f_nodes > 0 && (!f_nodes || !f_ptr || !f_feats))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (kf->device != F->device) { set_error("frames on different devices"); return YGZFE_EINVAL; }
    // ORBmatcher.cc:170-243: walk the two node-sorted FeatureVectors; every KF feature of
    // a shared node is one query over that node's F features
    MatchCall c;
    c.train = F;
    int KFit = 0, Fit = 0;
    while (KFit < n_kf_nodes && Fit < n_f_nodes) {
        if (kf_nodes[KFit] == f_nodes[Fit]) {
            for (int a = kf_ptr[KFit]; a < kf_ptr[KFit + 1]; a++) {
                const int idx = kf_feats[a];
                if (idx < 0 || idx >= kf->n) { set_error("KF feature index %d out of range", idx); return YGZFE_EINVAL; }
                ygzfe_match_query Q;
                memset(&Q, 0, sizeof(Q));
                Q.angle = kf->host_kps[idx].angle;
                Q.min_level = Q.max_level = -1;
                Q.flags = kf_usable[idx] ? YGZFE_MQ_VALID : 0;
                c.q.push_back(Q);
                c.qid.push_back(idx);
                c.cand_ptr.push_back(f_ptr[Fit]);
                c.cand_ptr.push_back(f_ptr[Fit + 1]);
            }
            KFit++;
            Fit++;
        } else if (kf_nodes[KFit] < f_nodes[Fit]) {
            KFit = (int)(std::lower_bound(kf_nodes + KFit, kf_nodes + n_kf_nodes, f_nodes[Fit]) - kf_nodes);
        } else {
            Fit = (int)(std::lower_bound(f_nodes + Fit, f_nodes + n_f_nodes, kf_nodes[KFit]) - f_nodes);
        }
    }
    const int n_cand = n_f_nodes > 0 ? f_ptr[n_f_nodes] : 0;
    for (int i = 0; i < n_cand; i++)
        if (f_feats[i] < 0 || f_feats[i] >= F->n) { set_error("F feature index %d out of range", f_feats[i]); return YGZFE_EINVAL; }
    c.cand_host = f_feats;
    c.n_cand = n_cand;
    if (c.cand_ptr.empty()) c.cand_ptr.assign(2, 0);  // BoW mode even with no query
    c.qdesc_dev = kf->desc.as<uint8_t>();
    c.qframe = kf;
    c.mode = YGZFE_MATCH_BOW;
    c.nnratio = nnratio;
    c.check_ori = check_ori;
    c.train_out = f_match;
    YGZ_TRY(run_match(c));
    *nmatches = c.nmatches;
    return YGZFE_OK;
}

// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:597-746) for all neighbours of one keyframe: the node
// walks and the argument checks on the host, then one packed H2D, k_tri_search + k_tri_votes, one D2H.
extern "C" int ygzfe_search_for_triangulation_batch(
    ygzfe_match_frame *kf1, const uint8_t *has_mp1, int n1_nodes, const int32_t *nodes1, const int32_t *ptr1,
    const int32_t *feats1, int n_nb, ygzfe_match_frame *const *kf2, const int32_t *mp2_ptr, const uint8_t *has_mp2,
    const int32_t *fv2_ptr, const int32_t *nodes2, const int32_t *ptr2, const int32_t *feats2, const float *F12,
    const float *epipole, const float *level_sigma2, const float *scale_factors, int n_levels, int only_stereo,
    int check_ori, int32_t *matches12, int32_t *nmatches) {
    if (!kf1 || n_nb < 0 || n1_nodes < 0 || n_levels <= 0 || !level_sigma2 || !scale_factors ||
        (kf1->n > 0 && !has_mp1) || (n1_nodes > 0 && (!nodes1 || !ptr1)) ||
        (n_nb > 0 && (!kf2 || !mp2_ptr || !fv2_ptr || !F12 || !epipole || !nmatches || (kf1->n > 0 && !matches12)))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (n_nb == 0) return YGZFE_OK;
    const int n1 = kf1->n;
    // KF1's FeatureVector: ranges in order, every feature in range and in one node only (DBoW2: one node per feature)
    const int n_feats1 = n1_nodes > 0 ? ptr1[n1_nodes] : 0;
    if (n1_nodes > 0 && (ptr1[0] != 0 || n_feats1 < 0 || (n_feats1 > 0 && !feats1))) {
        set_error("KF1 FeatureVector: ptr1 must start at 0 and feats1 be given");
        return YGZFE_EINVAL;
    }
    for (int k = 0; k < n1_nodes; k++)
        if (ptr1[k] > ptr1[k + 1]) { set_error("KF1 FeatureVector: ptr1 decreases at node %d", k); return YGZFE_EINVAL; }
    std::vector<uint8_t> seen1((size_t)n1, 0);
    for (int a = 0; a < n_feats1; a++) {
        const int idx = feats1[a];
        if (idx < 0 || idx >= n1) { set_error("KF1 feature index %d out of range", idx); return YGZFE_EINVAL; }
        if (seen1[idx]) { set_error("KF1 feature %d is listed in two nodes", idx); return YGZFE_EINVAL; }
        seen1[idx] = 1;
    }
    if (mp2_ptr[0] != 0 || fv2_ptr[0] != 0) { set_error("mp2_ptr and fv2_ptr must start at 0"); return YGZFE_EINVAL; }
    for (int k = 0; k < n_nb; k++) {
        const ygzfe_match_frame *f = kf2[k];
        if (!f) { set_error("neighbour %d is null", k); return YGZFE_EINVAL; }
        if (f->device != kf1->device) { set_error("frames on different devices"); return YGZFE_EINVAL; }
        if (mp2_ptr[k + 1] - mp2_ptr[k] != f->n) {
            set_error("neighbour %d: has_mp2 holds %d rows for %d keypoints", k, mp2_ptr[k + 1] - mp2_ptr[k], f->n);
            return YGZFE_EINVAL;
        }
        if (fv2_ptr[k + 1] < fv2_ptr[k]) { set_error("fv2_ptr decreases at neighbour %d", k); return YGZFE_EINVAL; }
        for (int i = 0; i < f->n; i++)  // level_sigma2 / scale_factors are indexed by any candidate's octave
            if (f->host_kps[i].octave < 0 || f->host_kps[i].octave >= n_levels) {
                set_error("neighbour %d keypoint %d: octave %d outside [0, %d)", k, i, f->host_kps[i].octave, n_levels);
                return YGZFE_EINVAL;
            }
    }
    const int n2_nodes = fv2_ptr[n_nb], n_feats2 = n2_nodes > 0 && ptr2 ? ptr2[n2_nodes] : 0;
    if ((mp2_ptr[n_nb] > 0 && !has_mp2) || (n2_nodes > 0 && (!nodes2 || !ptr2)) || n_feats2 < 0 ||
        (n_feats2 > 0 && !feats2) || (n2_nodes > 0 && ptr2[0] != 0)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    for (int k = 0; k < n_nb; k++)
        for (int j = fv2_ptr[k]; j < fv2_ptr[k + 1]; j++) {
            if (ptr2[j] > ptr2[j + 1]) { set_error("neighbour %d FeatureVector: ptr2 decreases", k); return YGZFE_EINVAL; }
            for (int a = ptr2[j]; a < ptr2[j + 1]; a++)
                if (feats2[a] < 0 || feats2[a] >= kf2[k]->n) {
                    set_error("neighbour %d feature index %d out of range", k, feats2[a]);
                    return YGZFE_EINVAL;
                }
        }
    // :625-716 per neighbour: the lower-bound merge of the two node lists; every KF1 feature of a shared
    // node without a MapPoint (:638) is one row over that node's KF2 features
    std::vector<TriRow> rows;
    for (int k = 0; k < n_nb; k++) {
        const int32_t *n2 = nodes2 + fv2_ptr[k], *p2 = ptr2 + fv2_ptr[k];
        const int m2 = fv2_ptr[k + 1] - fv2_ptr[k];
        int it1 = 0, it2 = 0;
        while (it1 < n1_nodes && it2 < m2) {
            if (nodes1[it1] == n2[it2]) {
                if (p2[it2 + 1] > p2[it2])
                    for (int a = ptr1[it1]; a < ptr1[it1 + 1]; a++)
                        if (!has_mp1[feats1[a]]) rows.push_back(TriRow{k, feats1[a], p2[it2], p2[it2 + 1]});
                it1++;
                it2++;
            } else if (nodes1[it1] < n2[it2]) {
                it1 = (int)(std::lower_bound(nodes1 + it1, nodes1 + n1_nodes, n2[it2]) - nodes1);
            } else {
                it2 = (int)(std::lower_bound(n2 + it2, n2 + m2, nodes1[it1]) - n2);
            }
        }
    }
    const size_t n_out = (size_t)n_nb * n1;
    if (rows.empty()) {  // nothing to search: no device work
        std::fill(matches12, matches12 + n_out, -1);
        std::fill(nmatches, nmatches + n_nb, 0);
        return YGZFE_OK;
    }
    StagingLease S;
    YGZ_TRY(S.acquire(kf1->device));
    // in: [neighbour table][rows][feats2][sigma2][scale][has_mp2]   out: [matches12 n_nb x n1][nmatches n_nb]
    BlockLayout in{16}, out{16};
    const size_t o_nb = in.take(n_nb, sizeof(TriNeighbour)), o_rows = in.take(rows.size(), sizeof(TriRow));
    const size_t o_f2 = in.take(n_feats2, 4), o_sig = in.take(n_levels, 4), o_sc = in.take(n_levels, 4);
    const size_t o_mp = in.take(std::max(mp2_ptr[n_nb], 1)), in_bytes = in.size();
    const size_t o_m = out.take(n_out, 4), o_nm = out.take(n_nb, 4), out_bytes = out.size();
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>(), *dout = d + in_bytes;
    TriNeighbour *tab = at<TriNeighbour>(h, o_nb);
    // the frames' uploads (ygzfe_match_frame_set is asynchronous on each frame's own stream) come first
    if (kf1->ev_ready) YGZ_HIP(hipStreamWaitEvent(S->stream, kf1->ev_ready, 0));
    for (int k = 0; k < n_nb; k++) {
        const ygzfe_match_frame *f = kf2[k];
        if (f->ev_ready) YGZ_HIP(hipStreamWaitEvent(S->stream, f->ev_ready, 0));
        TriNeighbour &N = tab[k];
        N.kps = f->kps.as<ygzfe_kp>();
        N.desc = f->desc.as<uint8_t>();
        N.u_right = f->has_uright ? f->uright.as<float>() : nullptr;
        N.mp_off = mp2_ptr[k];
        memcpy(N.F, F12 + 9 * (size_t)k, sizeof(N.F));
        N.ex = epipole[2 * k];
        N.ey = epipole[2 * k + 1];
    }
    memcpy(h + o_rows, rows.data(), rows.size() * sizeof(TriRow));
    memcpy(h + o_f2, feats2, (size_t)n_feats2 * 4);
    memcpy(h + o_sig, level_sigma2, (size_t)n_levels * 4);
    memcpy(h + o_sc, scale_factors, (size_t)n_levels * 4);
    if (mp2_ptr[n_nb] > 0) memcpy(h + o_mp, has_mp2, (size_t)mp2_ptr[n_nb]);
    YGZ_TRY(S.upload(in_bytes));
    TriJob J;
    J.kps1 = kf1->kps.as<ygzfe_kp>();
    J.desc1 = kf1->desc.as<uint8_t>();
    J.u_right1 = kf1->has_uright ? kf1->uright.as<float>() : nullptr;
    J.n1 = n1;
    J.n_nb = n_nb;
    J.n_rows = (int)rows.size();
    J.nb = at<const TriNeighbour>(d, o_nb);
    J.rows = at<const TriRow>(d, o_rows);
    J.feats2 = at<const int32_t>(d, o_f2);
    J.has_mp2 = d + o_mp;
    J.level_sigma2 = at<const float>(d, o_sig);
    J.scale_factors = at<const float>(d, o_sc);
    J.only_stereo = only_stereo != 0;
    J.check_ori = check_ori != 0;
    J.matches12 = at<int32_t>(dout, o_m);
    J.nmatches = at<int32_t>(dout, o_nm);
    YGZ_HIP(hipMemsetAsync(J.matches12, 0xFF, n_out * 4, S->stream));  // -1: vMatches12's initial value (:617)
    YGZ_HIP(launch_triangulation(J, S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    memcpy(matches12, S->hout.as<uint8_t>() + o_m, n_out * 4);
    memcpy(nmatches, S->hout.as<uint8_t>() + o_nm, (size_t)n_nb * 4);
    return YGZFE_OK;
}

extern "C" int ygzfe_search_for_triangulation(
    ygzfe_match_frame *kf1, const uint8_t *has_mp1, int n1_nodes, const int32_t *nodes1, const int32_t *ptr1,
    const int32_t *feats1, ygzfe_match_frame *kf2, const uint8_t *has_mp2, int n2_nodes, const int32_t *nodes2,
    const int32_t *ptr2, const int32_t *feats2, const float *F12, const float *epipole, const float *level_sigma2,
    const float *scale_factors, int n_levels, int only_stereo, int check_ori, int32_t *matches12, int32_t *nmatches) {
    if (!kf2 || n2_nodes < 0) { set_error("invalid argument"); return YGZFE_EINVAL; }
    const int32_t mp2_ptr[2] = {0, kf2->n}, fv2_ptr[2] = {0, n2_nodes};
    return ygzfe_search_for_triangulation_batch(kf1, has_mp1, n1_nodes, nodes1, ptr1, feats1, 1, &kf2, mp2_ptr, has_mp2,
                                                fv2_ptr, nodes2, ptr2, feats2, F12, epipole, level_sigma2,
                                                scale_factors, n_levels, only_stereo, check_ori, matches12, nmatches);
}

// MapPoint::PredictScale (MapPoint.cc:343-357) as a table: nScale >= L  <=>  ratio >= thr[L - 1].  Positive
// floats are ordered like their bit patterns, so the smallest one that reaches level L is found by bisection
// over the bits, evaluating the reference's own expression (float logf, float divide, float ceil).
namespace {
bool reaches_level(float ratio, float log_scale_factor, int L) {
    return ceilf(logf(ratio) / log_scale_factor) >= (float)L;
}
float bits_float(uint32_t b) {
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}
}  // namespace

extern "C" int ygzfe_predict_scale_thresholds(float log_scale_factor, int n_levels, float *thr) {
    if (!thr || n_levels < 1 || n_levels > 16 || !(log_scale_factor > 0.0f) || !std::isfinite(log_scale_factor)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    for (int L = 1; L < n_levels; L++) {
        uint32_t lo = 1u, hi = 0x7F7FFFFFu;  // smallest subnormal .. FLT_MAX
        if (!reaches_level(bits_float(hi), log_scale_factor, L)) {
            thr[L - 1] = INFINITY;  // no finite ratio reaches the level
            continue;
        }
        if (reaches_level(bits_float(lo), log_scale_factor, L)) hi = lo;
        while (hi - lo > 1) {  // !reaches(lo) && reaches(hi)
            const uint32_t mid = lo + (hi - lo) / 2;
            (reaches_level(bits_float(mid), log_scale_factor, L) ? hi : lo) = mid;
        }
        thr[L - 1] = bits_float(hi);
    }
    return YGZFE_OK;
}

// ORBmatcher::Fuse's search for n_kf keyframes x n_pts map points: the argument checks and the threshold
// table on the host, then one packed H2D, k_fuse_search, one D2H.
extern "C" int ygzfe_fuse_search_batch(int n_kf, ygzfe_match_frame *const *kf, const float *view, int n_pts,
                                       const float *world, const float *normal, const float *min_dist,
                                       const float *max_dist, const uint8_t *desc, const uint8_t *skip, float th,
                                       const float *scale_factors, const float *inv_level_sigma2, int n_levels,
                                       float log_scale_factor, int check_reproj, int32_t *best_idx,
                                       int32_t *best_dist) {
    if (n_kf < 0 || n_pts < 0 || !scale_factors || !inv_level_sigma2 || (n_kf > 0 && (!kf || !view)) ||
        (n_pts > 0 && (!world || !normal || !min_dist || !max_dist || !desc)) ||
        (n_kf > 0 && n_pts > 0 && (!best_idx || !best_dist))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (n_levels < 1 || n_levels > 16) { set_error("n_levels %d outside [1, 16]", n_levels); return YGZFE_EINVAL; }
    if (!(log_scale_factor > 0.0f) || !std::isfinite(log_scale_factor)) {
        set_error("log_scale_factor must be finite and positive");
        return YGZFE_EINVAL;
    }
    if ((long long)n_kf * n_pts > (1ll << 30)) { set_error("%d x %d pairs exceed 2^30", n_kf, n_pts); return YGZFE_EINVAL; }
    for (int k = 0; k < n_kf; k++) {
        const ygzfe_match_frame *f = kf[k];
        if (!f) { set_error("keyframe %d is null", k); return YGZFE_EINVAL; }
        if (f->device != kf[0]->device) { set_error("frames on different devices"); return YGZFE_EINVAL; }
        for (int i = 0; i < f->n; i++)  // the level filter and inv_level_sigma2 are indexed by the octave
            if (f->host_kps[i].octave < 0 || f->host_kps[i].octave >= n_levels) {
                set_error("keyframe %d keypoint %d: octave %d outside [0, %d)", k, i, f->host_kps[i].octave, n_levels);
                return YGZFE_EINVAL;
            }
    }
    if (n_kf == 0 || n_pts == 0) return YGZFE_OK;
    float thr[16] = {0};  // all 16 are uploaded
    YGZ_TRY(ygzfe_predict_scale_thresholds(log_scale_factor, n_levels, thr));
    StagingLease S;
    YGZ_TRY(S.acquire(kf[0]->device));
    // in: [keyframe table][desc][world][normal][min][max][thr][scale][inv sigma2][skip]   out: [best_idx][best_dist]
    const size_t n_out = (size_t)n_kf * n_pts;
    BlockLayout in{16}, out{16};
    const size_t o_kf = in.take(n_kf, sizeof(FuseKf)), o_d = in.take(n_pts, 32), o_w = in.take(n_pts, 12);
    const size_t o_n = in.take(n_pts, 12), o_mn = in.take(n_pts, 4), o_mx = in.take(n_pts, 4), o_thr = in.take(16, 4);
    const size_t o_sc = in.take(n_levels, 4), o_sig = in.take(n_levels, 4), o_sk = skip ? in.take(n_out) : 0;
    const size_t in_bytes = in.size();
    const size_t o_bi = out.take(n_out, 4), o_bd = out.take(n_out, 4), out_bytes = out.size();
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>(), *dout = d + in_bytes;
    FuseKf *tab = at<FuseKf>(h, o_kf);
    for (int k = 0; k < n_kf; k++) {
        const ygzfe_match_frame *f = kf[k];
        // the frame's upload and grid (asynchronous on its own stream) come first
        if (f->ev_ready) YGZ_HIP(hipStreamWaitEvent(S->stream, f->ev_ready, 0));
        FuseKf &K = tab[k];
        K.kps = f->kps.as<ygzfe_kp>();
        K.desc = f->desc.as<uint8_t>();
        K.u_right = f->has_uright ? f->uright.as<float>() : nullptr;
        K.cend = f->cell.as<int32_t>() + f->n;
        K.cidx = reinterpret_cast<const uint16_t *>(K.cend + kMatchCells);
        K.n = f->n;
        K.min_x = f->bounds.min_x;
        K.max_x = f->bounds.max_x;
        K.min_y = f->bounds.min_y;
        K.max_y = f->bounds.max_y;
        K.inv_w = f->inv_w;
        K.inv_h = f->inv_h;
        memcpy(K.view, view + 20 * (size_t)k, sizeof(K.view));
    }
    memcpy(h + o_d, desc, (size_t)n_pts * 32);
    memcpy(h + o_w, world, (size_t)n_pts * 12);
    memcpy(h + o_n, normal, (size_t)n_pts * 12);
    memcpy(h + o_mn, min_dist, (size_t)n_pts * 4);
    memcpy(h + o_mx, max_dist, (size_t)n_pts * 4);
    memcpy(h + o_thr, thr, sizeof(thr));
    memcpy(h + o_sc, scale_factors, (size_t)n_levels * 4);
    memcpy(h + o_sig, inv_level_sigma2, (size_t)n_levels * 4);
    if (skip) memcpy(h + o_sk, skip, n_out);
    YGZ_TRY(S.upload(in_bytes));
    FuseJob J;
    J.kf = at<const FuseKf>(d, o_kf);
    J.n_kf = n_kf;
    J.n_pts = n_pts;
    J.world = at<const float>(d, o_w);
    J.normal = at<const float>(d, o_n);
    J.min_dist = at<const float>(d, o_mn);
    J.max_dist = at<const float>(d, o_mx);
    J.desc = d + o_d;
    J.skip = skip ? d + o_sk : nullptr;
    J.thr = at<const float>(d, o_thr);
    J.scale_factors = at<const float>(d, o_sc);
    J.inv_level_sigma2 = at<const float>(d, o_sig);
    J.th = th;
    J.n_levels = n_levels;
    J.check_reproj = check_reproj != 0;
    J.best_idx = at<int32_t>(dout, o_bi);
    J.best_dist = at<int32_t>(dout, o_bd);
    YGZ_HIP(launch_fuse_search(J, S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    memcpy(best_idx, S->hout.as<uint8_t>() + o_bi, n_out * 4);
    memcpy(best_dist, S->hout.as<uint8_t>() + o_bd, n_out * 4);
    return YGZFE_OK;
}

extern "C" int ygzfe_fuse_search(ygzfe_match_frame *kf, const float *view, int n_pts, const float *world,
                                 const float *normal, const float *min_dist, const float *max_dist,
                                 const uint8_t *desc, const uint8_t *skip, float th, const float *scale_factors,
                                 const float *inv_level_sigma2, int n_levels, float log_scale_factor,
                                 int check_reproj, int32_t *best_idx, int32_t *best_dist) {
    if (!kf) { set_error("invalid argument"); return YGZFE_EINVAL; }
    return ygzfe_fuse_search_batch(1, &kf, view, n_pts, world, normal, min_dist, max_dist, desc, skip, th,
                                   scale_factors, inv_level_sigma2, n_levels, log_scale_factor, check_reproj,
                                   best_idx, best_dist);
}
