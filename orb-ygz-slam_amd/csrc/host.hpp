// host.hpp — what the host files of the C ABI (include/ygzfe.h over the gfx950 kernels) share:
// host.cpp and the api_*.cpp files, one per subsystem.
//
// Host-side responsibilities only: planning (plan.cpp), device buffers,
// stream ordering and H2D/D2H of the host-pointer entry points.  No compute
// happens on the host; there is no CPU fallback.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "kernels.hpp"
#include "plan.hpp"
#include "staging.hpp"

namespace ygzfe {

int ensure_device(int device);

// Graph capture vs. teardown across threads: a thread capturing its extraction
// graph must not overlap another thread's hipFree / stream / graph destruction (the
// runtime's capture bookkeeping is process-wide; tests/test_gpu_concurrency.py hit it
// with two extractors on two threads, Frame.cc:728-731).  Capture takes ~0.1 ms once
// per frame handle; teardown is rare: one lock for both.
std::recursive_mutex &graph_mutex();

struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && owned) {
            std::lock_guard<std::recursive_mutex> lk(graph_mutex());  // not during another thread's capture
            (void)hipFree(p);
        }
        p = nullptr;
        n = 0;
        owned = true;
    }
    int ensure(size_t bytes) {
        if (p && n >= bytes) return YGZFE_OK;
        release();
        if (bytes == 0) bytes = 16;
        std::lock_guard<std::recursive_mutex> lk(graph_mutex());
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc(%zu) failed", bytes);
            return YGZFE_ENOMEM;
        }
        n = bytes;
        // YGZFE_POISON=1 (debugging): fresh buffers start as 0xA5 bytes instead of whatever
        // the allocator hands back, so a read-before-write shows on every run
        static const bool poison = getenv("YGZFE_POISON") != nullptr;
        if (poison) (void)hipMemset(p, 0xA5, bytes);
        return YGZFE_OK;
    }
    void bind(void *ext, size_t bytes) {
        release();
        p = ext;
        n = bytes;
        owned = false;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// page-locked host staging (hipHostMalloc): one DMA per direction per call
// instead of a pageable copy per argument
struct HostBuf {
    void *p = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() {
        if (p) (void)hipHostFree(p);
    }
    int ensure(size_t bytes) {
        if (p && n >= bytes) return YGZFE_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        bytes = std::max<size_t>(bytes, 4096);
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            set_error("hipHostMalloc(%zu) failed", bytes);
            return YGZFE_ENOMEM;
        }
        n = bytes;
        return YGZFE_OK;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

#define YGZ_TRY(x)                          \
    do {                                    \
        int r_ = (x);                       \
        if (r_ != YGZFE_OK) return r_;      \
    } while (0)

// Host entry points without a handle (Hamming, RGB-D depth lookup, Align2D on a host
// image, FAST-10 ROIs): a call leases a staging area from a process-wide pool per
// device -- its own non-blocking stream, a device buffer and pinned in / out buffers
// that only grow -- and returns it when the call ends, so a call is one packed H2D,
// the launches, one packed D2H and one stream synchronisation (no allocation, no
// device-wide synchronisation).  The pool holds as many areas as calls ever ran at
// once, whatever the number of threads that come and go (no per-thread leak).
struct CallStaging {
    hipStream_t stream = nullptr;
    DevBuf dev;
    HostBuf hin, hout;
};
std::mutex &staging_mutex();
std::map<int, std::vector<CallStaging *>> &staging_free();
struct StagingLease {
    CallStaging *s = nullptr;
    int device = -1;
    StagingLease() = default;
    StagingLease(const StagingLease &) = delete;
    StagingLease &operator=(const StagingLease &) = delete;
    ~StagingLease() {
        if (!s) return;
        // an early error return may leave DMAs into / out of the pinned buffers queued:
        // the next lessee (possibly another thread) writes them at once
        if (hipStreamQuery(s->stream) != hipSuccess) (void)hipStreamSynchronize(s->stream);
        std::lock_guard<std::mutex> lk(staging_mutex());
        staging_free()[device].push_back(s);
    }
    CallStaging *operator->() const { return s; }
    int acquire(int dev) {
        YGZ_TRY(ensure_device(dev));
        device = dev;
        {
            std::lock_guard<std::mutex> lk(staging_mutex());
            std::vector<CallStaging *> &fl = staging_free()[dev];
            if (!fl.empty()) {
                s = fl.back();
                fl.pop_back();
                return YGZFE_OK;
            }
        }
        CallStaging *n = new CallStaging();
        if (hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking) != hipSuccess) {
            delete n;
            set_error("hipStreamCreate failed");
            return YGZFE_EHIP;
        }
        s = n;
        return YGZFE_OK;
    }
    // a packed call of `in` bytes up and `out` bytes back, on the device [in][out]: reserve(), fill hin,
    // upload(), the launches, download() into hout
    int reserve(size_t in, size_t out) {
        YGZ_TRY(s->hin.ensure(in));
        YGZ_TRY(s->hout.ensure(out));
        return s->dev.ensure(in + out);
    }
    int upload(size_t in) {
        YGZ_HIP(hipMemcpyAsync(s->dev.p, s->hin.p, in, hipMemcpyHostToDevice, s->stream));
        return YGZFE_OK;
    }
    int download(size_t in, size_t out) {
        YGZ_HIP(hipMemcpyAsync(s->hout.p, at<uint8_t>(s->dev.p, in), out, hipMemcpyDeviceToHost, s->stream));
        YGZ_HIP(hipStreamSynchronize(s->stream));
        return YGZFE_OK;
    }
};

struct PlanDev {
    PlanHost host;
    DevBuf plan, cells, tabs;
    int upload();
    const Plan &hp() const { return host.plan; }
    const Plan *dp() const { return plan.as<Plan>(); }
};

int make_plan(const ygzfe_orb_params &p, int W, int H, std::unique_ptr<PlanDev> *out);

// extraction scratch for F frames of one plan
struct Workspace {
    int F = 0, rows = 0;
    DevBuf blur, cellbuf, cellcnt, candA, candB, sel, selcnt, kps, desc, counts, nexist, err, ojobs, octq;
    DevBuf occ, dso_keys, dso_cnt, dso_total;
    int ensure(const Plan &P, int frames, int rows_needed) {
        F = frames;
        rows = rows_needed;
        YGZ_TRY(blur.ensure((size_t)F * P.pyr_bytes));
        YGZ_TRY(cellbuf.ensure((size_t)F * P.ncells * P.cell_cap * 4 + 16));
        YGZ_TRY(cellcnt.ensure((size_t)F * P.ncells * 4 + 16));
        YGZ_TRY(candA.ensure((size_t)F * P.cand_total * 8 + 16));
        YGZ_TRY(candB.ensure((size_t)F * P.cand_total * 8 + 16));
        YGZ_TRY(sel.ensure((size_t)F * P.sel_total * 4 + 16));
        YGZ_TRY(ojobs.ensure((size_t)F * P.sel_total * 8 + 16));
        YGZ_TRY(selcnt.ensure((size_t)F * P.nlevels * 4 + 128));  // tail: k_orient_desc's 8-int scalar load
        YGZ_TRY(kps.ensure((size_t)F * rows * sizeof(ygzfe_kp) + 16));
        YGZ_TRY(desc.ensure((size_t)F * rows * 32 + 16));
        YGZ_TRY(counts.ensure((size_t)F * 4 + 16));
        YGZ_TRY(nexist.ensure((size_t)F * 4 + 16));
        YGZ_TRY(err.ensure(16));
        YGZ_TRY(octq.ensure(octree_queue_ints(P, F) * sizeof(int)));
        return YGZFE_OK;
    }
};

}  // namespace ygzfe

using namespace ygzfe;

// --------------------------------------------------------------------------- handles
struct ygzfe_extractor {
    ygzfe_orb_params p;
    int device = 0;
    // frames borrow the extractor (its stream, mutex, plans): a destroy while frames are
    // alive is deferred to the last frame's destroy (under graph_mutex())
    int live_frames = 0;
    bool dead = false;
    hipStream_t stream = nullptr;
    ScaleInfo scales;
    std::map<std::pair<int, int>, std::unique_ptr<PlanDev>> plans;
    Workspace ws;
    int dso_grid = -1;
    // SearchLocalPointsDirect staging: one packed H2D, one packed D2H per call
    DevBuf direct_dev;
    HostBuf direct_hin, direct_hout;
    // single-frame latency path: side streams (side[0] the blur, side[1] the octree
    // classes after the first under YGZFE_OCT_FORK) forked from / joined to `stream`, pinned staging,
    // the packed extraction result (one D2H) and the SparseImgAlign buffers
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_oct_fork = nullptr, ev_oct_join[2] = {nullptr, nullptr};
    HostBuf hin, hout, himg;
    hipEvent_t ev_img = nullptr;  // the last image DMA out of himg
    DevBuf res, align_in, align_scratch, align_out;
    // SparseImgAlign in flight (ygzfe_sparse_align_begin / _end): its own stream,
    // pinned staging and completion event, so it overlaps the same frame's extraction
    hipStream_t astream = nullptr;
    hipEvent_t ev_align_fork = nullptr, ev_align_done = nullptr;
    HostBuf ahin, ahout;
    HostBuf hlvl;  // page-locked staging of ygzfe_frame_level / _set_level (pageable 2-D copies are row by row)
    bool align_pending = false;
    bool graph_broken = false;  // stream capture failed once: plain launches
    std::mutex mu;
    // -1 when neither `stream` nor a side stream is in a capture, else the first that is
    // (0: stream, 1..3: side[0..2])
    int capture_left_open() const {
        const hipStream_t all[4] = {stream, side[0], side[1], side[2]};
        for (int i = 0; i < 4; i++) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (all[i] && (hipStreamIsCapturing(all[i], &cs) != hipSuccess || cs != hipStreamCaptureStatusNone))
                return i;
        }
        return -1;
    }
    int ensure_side();                                  // api_extract.cpp
    int probe_beside(hipStream_t cand, bool &beside);  // api_align.cpp
    int ensure_align_stream();                          // api_align.cpp
    int align_probe_attempts = 0;  // streams created by the placement probe (0: no align yet)
    int align_probe_beside = -1;   // 1: the align stream passed the probe; 0: taken unprobed
    // work about to rewrite a pyramid on `st` waits for the alignment reading it
    int order_after_align(hipStream_t st) {
        if (align_pending) YGZ_HIP(hipStreamWaitEvent(st, ev_align_done, 0));
        return YGZFE_OK;
    }
};

struct ygzfe_frame {
    ygzfe_extractor *ex = nullptr;
    PlanDev *plan = nullptr;
    int W = 0, H = 0;
    DevBuf pyr;
    // a keyframe's mvKeys (ygzfe_frame_set_keypoints), read by ygzfe_search_local_map_direct
    DevBuf kps;
    int n_kps = -1;
    // the captured single-frame extraction (ygzfe_extract, no existing rows)
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    const void *gkey[15] = {};
    int grows = 0;
    size_t gcopy = 0;
    void drop_graph() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        gexec = nullptr;
        graph = nullptr;
    }
    ~ygzfe_frame() { drop_graph(); }
};

struct ygzfe_batch {
    ygzfe_orb_params p;
    int device = 0;
    int maxF = 0;
    hipStream_t stream = nullptr;
    // fork/join inside one extract: the FAST levels >= 1 overlap level 0
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_oct_fork = nullptr, ev_oct_join[2] = {nullptr, nullptr};
    // end of the last extraction's descriptor pass (the last reader of the pyramid,
    // FAST / octree scratch): the next extraction and uploads wait on it
    hipEvent_t ev_desc_done = nullptr;
    bool desc_pending = false;
    std::unique_ptr<PlanDev> plan;
    DevBuf pyr;
    Workspace ws;
    // align scratch
    DevBuf jobs, ascratch, pairs_tmp;
    size_t ascratch_per_job = 0;
    // stereo scratch: jobs + winning SADs [pairs][kp_cap]
    DevBuf sjobs, ssad;
    // BoW scratch: per-feature word / weight / node [frames][kp_cap]
    DevBuf bow_word, bow_weight, bow_nid;
    // per-stage kernel timing with hipEvents on the launch stream (no sync while recording)
    bool timing = false;
    std::vector<hipEvent_t> pool;
    struct Rec { int stage; hipEvent_t a, b; };
    std::vector<Rec> pending;
    double total_ms[16] = {0};
    long calls[16] = {0};
    hipEvent_t get_event() {
        hipEvent_t e = nullptr;
        if (!pool.empty()) { e = pool.back(); pool.pop_back(); }
        else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        return e;
    }
    hipEvent_t begin(hipStream_t st) {
        if (!timing) return nullptr;
        hipEvent_t a = get_event();
        if (a) (void)hipEventRecord(a, st);
        return a;
    }
    void end(int stage, hipEvent_t a, hipStream_t st) {
        if (!timing || !a) return;
        hipEvent_t e = get_event();
        if (!e) return;
        (void)hipEventRecord(e, st);
        pending.push_back({stage, a, e});
    }
    int collect() {
        for (auto &r : pending) {
            float ms = 0.f;
            YGZ_HIP(hipEventSynchronize(r.b));
            YGZ_HIP(hipEventElapsedTime(&ms, r.a, r.b));
            total_ms[r.stage] += ms;
            calls[r.stage] += 1;
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        pending.clear();
        return YGZFE_OK;
    }
};

// the batch's timed stages (ygzfe_batch::begin / end; the names are with ygzfe_batch_timing)
enum { ST_PYR, ST_BLUR, ST_FAST, ST_OCT, ST_DESC, ST_HAM, ST_ALIGN, ST_STEREO, ST_PACK };

// helpers that one subsystem's file defines and another's calls
namespace ygzfe {
int pyramid_from_level0(ygzfe_frame *f, hipStream_t st);  // api_extract.cpp
int batch_wait(ygzfe_batch *b);                            // api_batch.cpp
AlignLevels levels_of(const Plan &P);                      // api_align.cpp
}  // namespace ygzfe
