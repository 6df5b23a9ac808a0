// plan_sweep.cpp — build_plan (csrc/plan.cpp) over image sizes and ORB parameters, without a GPU.
// A stand-alone host program linked with plan.cpp only, built with AddressSanitizer and UBSan
// (tests/test_cpu_plan_sweep.py): every accepted plan must be evaluated without undefined
// behaviour and hold the invariants the kernels rely on.  Prints the first violations and
// exits 1 if any; the last line counts accepted and rejected plans.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "plan.hpp"

using namespace ygzfe;

static int g_bad = 0;
static std::string g_ctx;
#define EXPECT(cond, ...)                                \
    do {                                                 \
        if (!(cond)) {                                   \
            if (g_bad++ < 20) {                          \
                printf("%s: %s: ", g_ctx.c_str(), #cond); \
                printf(__VA_ARGS__);                     \
                printf("\n");                            \
            }                                            \
        }                                                \
    } while (0)

// half-open int ranges [first, second) must not overlap
static bool disjoint(std::vector<std::pair<long, long>> r) {
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); i++)
        if (r[i].first < r[i - 1].second) return false;
    return true;
}

static void check_plan(const ygzfe_orb_params &p, int W, int H, const PlanHost &ph) {
    const Plan &P = ph.plan;
    EXPECT(P.W == W && P.H == H && P.nlevels == p.nlevels, "header %dx%d %d levels", P.W, P.H, P.nlevels);
    std::vector<std::pair<long, long>> pyr, sel, cand, tabs;
    long others = 0;
    int cells = 0, cell_cap = 1, need = 0;
    for (int l = 0; l < P.nlevels; l++) {
        const LevelDesc &L = P.lv[l];
        EXPECT(L.w >= 1 && L.h >= 1 && L.w < 4096 && L.h < 4096, "level %d size %dx%d", l, L.w, L.h);
        // level offsets: 16-byte aligned, one after the other inside pyr_bytes
        EXPECT(L.off % 16 == 0, "level %d offset %u", l, L.off);
        pyr.push_back({(long)L.off, (long)L.off + (long)L.w * L.h});
        EXPECT((long)L.off + (long)L.w * L.h <= (long)P.pyr_bytes, "level %d ends past pyr_bytes %u", l, P.pyr_bytes);
        // budgets: the levels before the last take cvRound of a geometric share, the last the rest,
        // clamped at 0 (ORBextractor.cc:434-445): the sum is nfeatures unless that clamp acted
        EXPECT(L.budget >= 0, "level %d budget %d", l, L.budget);
        if (l < P.nlevels - 1) others += L.budget;
        else EXPECT(L.budget == std::max((long)p.nfeatures - others, 0l), "last budget %d, others %ld", L.budget, others);
        EXPECT(L.sel_cap >= L.budget + 4, "level %d sel_cap %d budget %d", l, L.sel_cap, L.budget);
        sel.push_back({L.sel_off, L.sel_off + L.sel_cap});
        EXPECT(L.cand_cap >= 1, "level %d cand_cap %d", l, L.cand_cap);
        cand.push_back({L.cand_off, L.cand_off + L.cand_cap});
        // the candidate area and the octree roots
        const int aw = L.max_bx - kMinBorder, ah = L.max_by - kMinBorder;
        EXPECT(L.max_bx == L.w - kMinBorder && L.max_by == L.h - kMinBorder, "level %d borders", l);
        EXPECT(L.n_ini >= 1 && L.n_ini <= 8, "level %d n_ini %d", l, L.n_ini);
        EXPECT(isfinite(L.hX) && L.hX > 0, "level %d hX %g", l, (double)L.hX);
        EXPECT(L.oct_dn >= 1 && L.oct_rb >= 0 && L.oct_rb + 2 * L.oct_dn <= 32, "level %d rb %d dn %d", l, L.oct_rb,
               L.oct_dn);
        EXPECT((1 << L.oct_rb) >= L.n_ini && (L.oct_rb == 0 || (1 << (L.oct_rb - 1)) < L.n_ini), "level %d rb %d n_ini %d",
               l, L.oct_rb, L.n_ini);
        need = std::max(need, L.budget + 4 * L.n_ini + 16);
        if (aw > 0 && ah > 0) {
            // every index the kernels can form from a key: x <= aw into the x table, y <= ah into the y table
            EXPECT(L.hX * L.n_ini >= aw - 1 && L.hX * L.n_ini <= aw + 1, "level %d hX %g", l, (double)L.hX);
            EXPECT(L.oct_xtab >= 0 && L.oct_xtab + aw < (int)ph.tabs.size(), "level %d x table", l);
            EXPECT(L.oct_ytab >= 0 && L.oct_ytab + ah < (int)ph.tabs.size(), "level %d y table", l);
            tabs.push_back({L.oct_xtab, L.oct_xtab + aw + 1});
            tabs.push_back({L.oct_ytab, L.oct_ytab + ah + 1});
        } else {
            EXPECT(L.ncells == 0 && L.n_ini == 1 && L.oct_xtab == L.oct_ytab, "level %d without area: %d cells, n_ini %d",
                   l, L.ncells, L.n_ini);
        }
        if (L.resize_mode == 2) {
            tabs.push_back({L.xtab_off, L.xtab_off + 2 * L.w});
            tabs.push_back({L.ytab_off, L.ytab_off + 3 * L.h});
            EXPECT(L.ytab_off + 3 * L.h <= (int)ph.tabs.size() && L.xtab_off >= 0, "level %d resize tables", l);
        }
        // cells: this level's run of the cell list, each ROI inside the level and at most kMaxRoi
        EXPECT(L.cell_begin == cells && L.ncells >= 0, "level %d cell_begin %d after %d", l, L.cell_begin, cells);
        int rw = 0, rh = 0;
        for (int c = L.cell_begin; c < L.cell_begin + L.ncells && c < (int)ph.cells.size(); c++) {
            const CellDesc &cd = ph.cells[c];
            EXPECT(cd.level == l, "cell %d level %d in level %d", c, cd.level, l);
            EXPECT(cd.rw >= 7 && cd.rh >= 4 && cd.rw <= kMaxRoi && cd.rh <= kMaxRoi, "cell %d ROI %dx%d", c, cd.rw, cd.rh);
            EXPECT(cd.x0 >= 0 && cd.y0 >= 0 && cd.x0 + cd.rw <= L.w && cd.y0 + cd.rh <= L.h, "cell %d at %d,%d %dx%d", c,
                   cd.x0, cd.y0, cd.rw, cd.rh);
            EXPECT(cd.x0 + cd.rw <= L.max_bx && cd.y0 + cd.rh <= L.max_by, "cell %d past the border", c);
            // key coordinates (ROI pixel + offset) index the code tables
            EXPECT(cd.offx == cd.x0 - kMinBorder && cd.offy == cd.y0 - kMinBorder, "cell %d offsets", c);
            EXPECT(cd.offx + cd.rw - 1 <= aw && cd.offy + cd.rh - 1 <= ah, "cell %d keys past the tables", c);
            rw = std::max(rw, (int)cd.rw);
            rh = std::max(rh, (int)cd.rh);
            cell_cap = std::max(cell_cap, ((std::max(cd.rw - 6, 0) + 1) / 2) * ((std::max(cd.rh - 6, 0) + 1) / 2));
        }
        EXPECT(L.fast_rw == rw && L.fast_rh == rh, "level %d ROI maxima %dx%d vs %dx%d", l, L.fast_rw, L.fast_rh, rw, rh);
        cells += L.ncells;
    }
    EXPECT(cells == P.ncells && cells == (int)ph.cells.size(), "cells %d / %d / %zu", cells, P.ncells, ph.cells.size());
    EXPECT(P.cell_cap == cell_cap, "cell_cap %d vs %d", P.cell_cap, cell_cap);
    EXPECT(disjoint(pyr), "levels overlap");
    EXPECT(disjoint(sel) && sel.back().second <= P.sel_total && P.kp_cap == P.sel_total, "selection slots");
    EXPECT(disjoint(cand) && cand.back().second <= P.cand_total, "candidate slots");
    EXPECT(disjoint(tabs), "tables overlap");
    EXPECT(P.node_cap >= need && P.node_cap <= 2048, "node_cap %d need %d", P.node_cap, need);
}

int main() {
    long accepted = 0, rejected = 0;
    PlanHost ph;
    char err[256];
    auto run = [&](int W, int H, float sf, int nl, int nf) {
        const ygzfe_orb_params p = {nf, sf, nl, 20, 7, 0};
        char ctx[128];
        snprintf(ctx, sizeof(ctx), "%dx%d scale %g levels %d nfeatures %d", W, H, (double)sf, nl, nf);
        g_ctx = ctx;
        err[0] = 0;
        if (build_plan(p, W, H, &ph, err, sizeof(err)) != 0) {
            EXPECT(err[0] != 0, "rejected without a message");
            rejected++;
            return;
        }
        accepted++;
        check_plan(p, W, H, ph);
    };
    const float scales[4] = {1.05f, 1.2f, 1.5f, 2.0f};
    const int levels[5] = {1, 2, 4, 8, 16}, feats[4] = {0, 1, 100, 2000};
    // every size with every scale factor, the level count and budget rotating with the size
    for (int W = 8; W <= 140; W++)
        for (int H = 8; H <= 140; H++)
            for (int s = 0; s < 4; s++) run(W, H, scales[s], levels[(W + 2 * H + s) % 5], feats[(3 * W + H + s) % 4]);
    // every parameter combination on a coarse grid of sizes, and on large and extreme-aspect ones
    std::vector<std::pair<int, int>> sizes;
    for (int W = 8; W <= 140; W += 11)
        for (int H = 9; H <= 140; H += 13) sizes.push_back({W, H});
    const int extra[][2] = {{752, 480}, {640, 480}, {641, 479}, {1280, 720}, {1920, 1080}, {4095, 4095}, {4096, 64},
                            {4095, 540}, {4095, 600}, {4095, 8}, {8, 4095}, {33, 4000}, {64, 200}, {480, 96}, {400, 70},
                            {300, 33}, {33, 300}, {32, 32}, {8, 8}, {31, 200}, {200, 31}};
    for (auto &e : extra) sizes.push_back({e[0], e[1]});
    for (auto &wh : sizes)
        for (float sf : scales)
            for (int nl : levels)
                for (int nf : feats) run(wh.first, wh.second, sf, nl, nf);
    // parameters outside the domain are refused
    const ygzfe_orb_params bad[] = {{100, 1.0f, 4, 20, 7, 0}, {100, 1.2f, 0, 20, 7, 0}, {100, 1.2f, 17, 20, 7, 0},
                                    {-1, 1.2f, 4, 20, 7, 0}};
    g_ctx = "invalid parameters";
    for (auto &p : bad) EXPECT(build_plan(p, 640, 480, &ph, err, sizeof(err)) != 0, "accepted");
    const ygzfe_orb_params ok = {100, 1.2f, 1, 20, 7, 0};
    EXPECT(build_plan(ok, 7, 480, &ph, err, sizeof(err)) != 0 && build_plan(ok, 480, 7, &ph, err, sizeof(err)) != 0,
           "accepted a side of 7");
    printf("%ld plans accepted, %ld rejected, %d violations\n", accepted, rejected, g_bad);
    if (accepted < 50000 || rejected < 1000) {
        printf("the sweep lost its coverage\n");
        return 1;
    }
    return g_bad ? 1 : 0;
}
