// host.cpp — the one definition of everything process-wide in the host layer (the error
// string, the per-device set-up, the graph mutex, the staging pool), plan upload, and the
// entry points that belong to no subsystem.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "host.hpp"

namespace ygzfe {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static const int kPatternHost[1024] = {
#include "../../include/ygzfe_pattern.inc"
};

int ensure_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (the ygzfe product path has no CPU fallback)");
        return YGZFE_EHIP;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (%d devices)", device, n);
        return YGZFE_EINVAL;
    }
    YGZ_HIP(hipSetDevice(device));
    static std::mutex mu;
    static bool uploaded[64] = {false};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 64 && !uploaded[device]) {
        YGZ_HIP(upload_pattern(kPatternHost));
        uint32_t fails[2] = {0, 0};
        YGZ_HIP(run_arith_guard(fails));
        if (fails[0] || fails[1]) {
            set_error("arithmetic guard failed on device %d (f16 ordering: %u, cvRound: %u mismatches): the "
                      "library was built with flags that break its bit-exact paths (fast-math, denormal flush)",
                      device, fails[0], fails[1]);
            return YGZFE_EHIP;
        }
        uploaded[device] = true;
    }
    return YGZFE_OK;
}

std::recursive_mutex &graph_mutex() {
    static std::recursive_mutex mu;
    return mu;
}

std::mutex &staging_mutex() {
    static std::mutex mu;
    return mu;
}
std::map<int, std::vector<CallStaging *>> &staging_free() {
    static auto *pool = new std::map<int, std::vector<CallStaging *>>();  // lives with the process
    return *pool;
}

int PlanDev::upload() {
    YGZ_TRY(plan.ensure(sizeof(Plan)));
    YGZ_TRY(cells.ensure(sizeof(CellDesc) * (host.cells.size() + 1)));
    YGZ_TRY(tabs.ensure(sizeof(int) * host.tabs.size()));
    host.plan.dtabs = tabs.as<int32_t>();
    YGZ_HIP(hipMemcpy(plan.p, &host.plan, sizeof(Plan), hipMemcpyHostToDevice));
    if (!host.cells.empty())
        YGZ_HIP(hipMemcpy(cells.p, host.cells.data(), sizeof(CellDesc) * host.cells.size(), hipMemcpyHostToDevice));
    YGZ_HIP(hipMemcpy(tabs.p, host.tabs.data(), sizeof(int) * host.tabs.size(), hipMemcpyHostToDevice));
    return YGZFE_OK;
}

int make_plan(const ygzfe_orb_params &p, int W, int H, std::unique_ptr<PlanDev> *out) {
    std::unique_ptr<PlanDev> pd(new PlanDev());
    char err[256];
    if (build_plan(p, W, H, &pd->host, err, sizeof(err)) != 0) {
        set_error("%s", err);
        return YGZFE_EINVAL;
    }
    YGZ_TRY(pd->upload());
    *out = std::move(pd);
    return YGZFE_OK;
}

}  // namespace ygzfe

extern "C" {

const char *ygzfe_last_error(void) { return g_err; }

int ygzfe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ygzfe_descriptor_distance(const uint8_t *a, const uint8_t *b) {
    // ORBmatcher::DescriptorDistance (ORBmatcher.cc:1507-1523): host scalar helper.
    int d = 0;
    for (int i = 0; i < 32; i += 4) {
        uint32_t x, y;
        memcpy(&x, a + i, 4);
        memcpy(&y, b + i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

}  // extern "C"
