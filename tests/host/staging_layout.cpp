// BlockLayout / at<T>() of csrc/staging.hpp, without a GPU: built with
// -fsanitize=address,undefined and run by tests/test_cpu_staging.py.
//
// 1. the layouts of the host entry points of csrc/api_*.cpp, replayed take by take for a few
//    inputs, against offsets worked out by hand from the aligned sums these entry
//    points were first written with (a16(x) = x rounded up to 16, a256 to 256; the hand
//    sum stands in the comment beside each number, none is computed through the helper);
// 2. properties of any sequence of takes;
// 3. every part of a block of exactly the total size written and read back through at<T>().
#include <stdio.h>
#include <stdlib.h>

#include "staging.hpp"

using ygzfe::at;
using ygzfe::BlockLayout;

static int g_fail = 0;

#define EXPECT(got, want)                                                                             \
    do {                                                                                              \
        const size_t g_ = (got), w_ = (want);                                                         \
        if (g_ != w_) {                                                                               \
            printf("%s:%d: %s = %zu, expected %zu\n", __FILE__, __LINE__, #got, g_, w_);              \
            g_fail++;                                                                                 \
        }                                                                                             \
    } while (0)

// element sizes of the parts: usable / flags 1, int32 / float 4, xyz 12, ygzfe_kp and
// ygzfe_se3 28, a descriptor 32, DirectItem 52, ygzfe_match_query 32, a pointer 8;
// AlignJob and StereoJob 88, ygzfe_pose_opt_result 168
struct Xyz { float v[3]; };
struct Kp { float f[5]; int32_t i[2]; };
static_assert(sizeof(Xyz) == 12 && sizeof(Kp) == 28, "element sizes of the cases below");
static const size_t kKp = 28, kSe3 = 28, kItem = 52, kJob = 88, kQuery = 32, kPoseResult = 168, kMaxLevels = 16;

static const size_t kAligns[] = {16, 256};

static size_t floor1(size_t n) { return n > 0 ? n : 1; }

// ---------------------------------------------------------------- 1. the entry points
static void hamming_best2(size_t nq, size_t nt, size_t o_t, size_t in_bytes) {
    BlockLayout in{16};
    EXPECT(in.take(nq, 32), 0);
    EXPECT(in.take(floor1(nt), 32), o_t);
    EXPECT(in.size(), in_bytes);
}

static void hamming_csr(size_t nq, size_t nt, size_t nc, size_t o_t, size_t o_r, size_t o_c, size_t in_bytes) {
    BlockLayout in{16};
    EXPECT(in.take(nq, 32), 0);
    EXPECT(in.take(nt, 32), o_t);
    EXPECT(in.take(nq + 1, 4), o_r);
    EXPECT(in.take(nc, 4), o_c);
    EXPECT(in.size(), in_bytes);
}

static void sparse_align(size_t n, size_t o_k, size_t o_x, size_t o_u, size_t in_bytes) {
    BlockLayout in{16};
    EXPECT(in.take(kJob), 0);
    EXPECT(in.take(n, kKp), o_k);
    EXPECT(in.take(n, 12), o_x);
    EXPECT(in.take(n), o_u);
    EXPECT(in.size(), in_bytes);
}

static void align2d_batch(size_t n, size_t o_p, size_t o_x, size_t in_bytes, size_t out_bytes, size_t dev_bytes) {
    BlockLayout in{16}, out{16};
    EXPECT(in.take(n, 100), 0);
    EXPECT(in.take(n, 64), o_p);
    EXPECT(in.take(n, 8), o_x);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(n, 9), 0);
    EXPECT(out.end(), out_bytes);
    EXPECT(in.size() + out.size(), dev_bytes);
}

static void fast10(size_t img_b, size_t n_roi, size_t cap, size_t o_r, size_t in_bytes, size_t o_xy,
                   size_t out_bytes) {
    BlockLayout in{16}, out{16};
    EXPECT(in.take(img_b), 0);
    EXPECT(in.take(n_roi, 16), o_r);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(n_roi, 4), 0);
    EXPECT(out.take(n_roi * cap, 4), o_xy);
    EXPECT(out.end(), out_bytes);
}

// ygzfe_debug_dso_cells and undistort_host: [first][second] in one device block
static void two_parts(size_t first, size_t second, size_t o_second, size_t dev_bytes) {
    BlockLayout blk{16};
    EXPECT(blk.take(first), 0);
    EXPECT(blk.take(second), o_second);
    EXPECT(blk.end(), dev_bytes);
}

static void find_direct(size_t nref, size_t nlevels, size_t n, const size_t (&o)[6], size_t in_bytes,
                        size_t out_bytes, size_t dev_bytes) {
    BlockLayout in{16}, out{16};
    EXPECT(in.take(nref, 8), 0);
    EXPECT(in.take(nlevels, 4), o[0]);
    EXPECT(in.take(n, 4), o[1]);
    EXPECT(in.take(n, kKp), o[2]);
    EXPECT(in.take(n, 12), o[3]);
    EXPECT(in.take(n, kSe3), o[4]);
    EXPECT(in.take(n, 8), o[5]);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(n, 13), 0);
    EXPECT(out.end(), out_bytes);
    EXPECT(in.size() + out.size(), dev_bytes);
}

static void search_direct(size_t n_ref, size_t n_points, size_t n_items, size_t n_tab, const size_t (&i)[6],
                          size_t in_bytes, size_t back_bytes, size_t o_pxi, size_t o_ok, size_t out_bytes) {
    BlockLayout in{256}, out{256};
    EXPECT(in.take(floor1(n_ref), 8), i[0]);
    EXPECT(in.take(kMaxLevels, 4), i[1]);
    EXPECT(in.take(n_points + 1, 4), i[2]);
    EXPECT(in.take(n_points, 8), i[3]);
    EXPECT(in.take(n_items, kItem), i[4]);
    EXPECT(in.take(floor1(n_tab), kSe3), i[5]);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(16 + 16 * n_points), 0);  // hdr 16 | px_out 8 | matched 4 | status 4, packed
    EXPECT(out.end(), back_bytes);
    EXPECT(out.take(n_items, 8), o_pxi);
    EXPECT(out.take(n_items), o_ok);
    EXPECT(out.size(), out_bytes);
}

static void local_map(size_t n_kf, size_t N, size_t n_obs, size_t M, const size_t (&i)[15], size_t in_bytes,
                      size_t back_bytes, const size_t (&s)[12], size_t out_bytes) {
    const size_t nk = floor1(n_kf), nblk = (N + 255) / 256, sel = 8;
    BlockLayout in{256}, out{256};
    const size_t in_parts[15][2] = {{nk, 8}, {nk, 8}, {kMaxLevels, 4}, {nk, 8}, {nk, 48}, {nk, kSe3}, {nk, 1}, {N, 12},
                                    {N, 12}, {N, 4}, {N, 4}, {N + 1, 4}, {N, 1}, {n_obs, 4}, {n_obs, 4}};
    for (int k = 0; k < 15; k++) EXPECT(in.take(in_parts[k][0], in_parts[k][1]), i[k]);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(16 + 40 * N), 0);  // hdr 16 | status 4, px_out 8, kf 4, kp 4, proj 12, cos 4, dist 4, packed
    EXPECT(out.end(), back_bytes);
    const size_t out_parts[12][2] = {{N, 1}, {N, 4}, {nblk, 4}, {sel * N, 4}, {sel * N, 4}, {N + 1, 4},
                                     {4, 1}, {N, 8}, {N, 4}, {M, kItem}, {M, 8}, {M, 1}};
    for (int k = 0; k < 12; k++) EXPECT(out.take(out_parts[k][0], out_parts[k][1]), s[k]);
    EXPECT(out.size(), out_bytes);
}

static void stereo_matches(size_t nl, size_t nr, const size_t (&o)[6], size_t in_bytes, const size_t (&r)[3],
                           size_t total) {
    BlockLayout blk{256};
    EXPECT(blk.take(kJob), o[0]);
    EXPECT(blk.take(8), o[1]);
    EXPECT(blk.take(nl, kKp), o[2]);
    EXPECT(blk.take(nr, kKp), o[3]);
    EXPECT(blk.take(nl, 32), o[4]);
    EXPECT(blk.take(nr, 32), o[5]);
    EXPECT(blk.size(), in_bytes);
    for (int k = 0; k < 3; k++) EXPECT(blk.take(nl, 4), r[k]);
    EXPECT(blk.size(), total);
}

static void stereo_from_rgbd(size_t stride, size_t height, size_t n, size_t o_k, size_t in_bytes) {
    BlockLayout in{16};
    EXPECT(in.take(stride * height, 4), 0);
    EXPECT(in.take(n, kKp), o_k);
    EXPECT(in.size(), in_bytes);
}

static void bow_one(size_t n, const size_t (&o)[9], size_t total) {
    const size_t N = floor1(n), elem[8] = {32, 4, 8, 4, 4, 8, 4, 4};
    BlockLayout blk{256};
    for (int k = 0; k < 8; k++) EXPECT(blk.take(N, elem[k]), o[k]);
    EXPECT(blk.take(16), o[8]);
    EXPECT(blk.size(), total);
}

static void run_match(size_t nq, size_t n, bool all_parts, size_t n_cand, const size_t (&i)[6], size_t in_bytes,
                      const size_t (&o)[7], size_t back_bytes, size_t dev_bytes) {
    BlockLayout ai{256}, ao{256};
    EXPECT(ai.take(floor1(nq), kQuery), i[0]);
    EXPECT(all_parts ? ai.take(floor1(nq), 32) : 0, i[1]);
    EXPECT(all_parts ? ai.take(nq, 4) : 0, i[2]);
    EXPECT(all_parts ? ai.take(nq + 1, 4) : 0, i[3]);
    EXPECT(all_parts ? ai.take(floor1(n_cand), 4) : 0, i[4]);
    EXPECT(all_parts ? ai.take(floor1(n)) : 0, i[5]);
    EXPECT(ai.size(), in_bytes);
    EXPECT(ao.take(floor1(n), 4), o[0]);
    EXPECT(ao.take(floor1(nq), 4), o[1]);
    EXPECT(ao.take(4, 4), o[2]);
    EXPECT(ao.size(), back_bytes);
    EXPECT(ao.take(32 * floor1(nq), 8), o[3]);
    for (int k = 4; k < 7; k++) EXPECT(ao.take(floor1(nq), 4), o[k]);
    EXPECT(ao.size(), dev_bytes);
}

static void pose_optimization(size_t n, size_t n_levels, const size_t (&o)[8], size_t in_bytes, size_t o_flags,
                              size_t out_bytes) {
    const size_t rows = floor1(n);
    BlockLayout in{16}, out{16};
    EXPECT(in.take(8), 0);       // problem_ptr[2]
    EXPECT(in.take(16), o[0]);   // camera
    EXPECT(in.take(4), o[1]);    // bf
    EXPECT(in.take(kSe3), o[2]);
    EXPECT(in.take(n_levels, 4), o[3]);
    EXPECT(in.take(rows, kKp), o[4]);
    EXPECT(in.take(rows, 12), o[5]);
    EXPECT(in.take(rows, 4), o[6]);
    EXPECT(in.take(rows), o[7]);
    EXPECT(in.size(), in_bytes);
    EXPECT(out.take(kPoseResult), 0);
    EXPECT(out.take(rows), o_flags);
    EXPECT(out.size(), out_bytes);
}

static void reference_layouts() {
    // [nq*32][max(nt,1)*32]: nt = 0 takes the floor of one row
    hamming_best2(17, 0, /*544*/ 544, /*544+32*/ 576);
    hamming_best2(1, 17, 32, /*32+544*/ 576);
    // [nq*32][nt*32][(nq+1)*4][nc*4]
    hamming_csr(17, 1, 17, 544, /*544+32*/ 576, /*576+a16(72)=576+80*/ 656, /*656+a16(68)=656+80*/ 736);
    hamming_csr(1, 17, 1, 32, /*32+544*/ 576, /*576+a16(8)*/ 592, /*592+a16(4)*/ 608);
    // [job 88][n*28][n*12][n]: a16(88) = 96
    sparse_align(17, 96, /*96+a16(476)=96+480*/ 576, /*576+a16(204)=576+208*/ 784, /*784+a16(17)=784+32*/ 816);
    sparse_align(1, 96, /*96+32*/ 128, /*128+16*/ 144, /*144+16*/ 160);
    sparse_align(0, 96, 96, 96, 96);
    // in [n*100][n*64][n*8], out n*9, device in + a16(out)
    align2d_batch(17, /*a16(1700)*/ 1712, /*1712+1088*/ 2800, /*2800+a16(136)=2800+144*/ 2944, 153, /*2944+160*/ 3104);
    align2d_batch(1, /*a16(100)*/ 112, /*112+64*/ 176, /*176+16*/ 192, 9, /*192+16*/ 208);
    // 63 x 47 image: 2961 bytes, a16 = 2976.  in [image][n_roi*16], out [n_roi*4][n_roi*cap*4]
    fast10(2961, 17, 1, 2976, /*2976+272*/ 3248, /*a16(68)*/ 80, /*80+68*/ 148);
    fast10(2961, 1, 17, 2976, /*2976+16*/ 2992, 16, /*16+68*/ 84);
    fast10(2961, 17, 0, 2976, 3248, 80, /*no corner list*/ 80);
    // ygzfe_debug_dso_cells, 63 x 47, g = 7: 6 x 9 cells of 49 flags = 2646
    two_parts(2961, 2646, 2976, /*2976+2646*/ 5622);
    // undistort_host, 63 x 47: uint8 and float images
    two_parts(2961, 2961, 2976, /*2976+2961*/ 5937);
    two_parts(11844, 11844, /*a16(11844)*/ 11856, /*11856+11844*/ 23700);
    // in [nref*8][nlevels*4][n*4][n*28][n*12][n*28][n*8], out n*13
    find_direct(1, 4, 17, {16, /*16+16*/ 32, /*32+a16(68)*/ 112, /*112+480*/ 592, /*592+208*/ 800, /*800+480*/ 1280},
                /*1280+144*/ 1424, 221, /*1424+a16(221)=1424+224*/ 1648);
    find_direct(3, 8, 1, {/*a16(24)*/ 32, /*32+32*/ 64, /*64+16*/ 80, /*80+32*/ 112, /*112+16*/ 128, /*128+32*/ 160},
                /*160+16*/ 176, 13, /*176+16*/ 192);
    // search_direct_impl, one point without items and without keyframes: the floors of one
    // pointer and one T; in [ptr 8][scale 64][item_ptr 8][px 8][items 0][T 28]
    search_direct(0, 1, 0, 0, {0, 256, /*a256(256+64)*/ 512, /*a256(512+8)*/ 768, /*a256(768+8)*/ 1024, 1024},
                  /*a256(1024+28)*/ 1280, /*16+16*/ 32, 256, 256, 256);
    search_direct(17, 17, 17, 17,
                  {0, /*a256(136)*/ 256, 512, /*a256(512+72)*/ 768, /*a256(768+136)*/ 1024, /*a256(1024+884)*/ 2048},
                  /*a256(2048+476)*/ 2560, /*16+16*17*/ 288, /*a256(288)*/ 512, /*a256(512+136)*/ 768,
                  /*a256(768+17)*/ 1024);
    // ygzfe_search_local_map_direct: no keyframe (floor 1), one candidate, no observation, no item
    local_map(0, 1, 0, 0, {0, 256, 512, /*512+64*/ 768, 1024, /*1024+48*/ 1280, /*1280+28*/ 1536, /*1536+1*/ 1792, 2048,
                           2304, 2560, 2816, /*2816+8*/ 3072, /*3072+1*/ 3328, 3328},
              3328, /*16+40*/ 56, {256, 512, 768, 1024, /*1024+32*/ 1280, /*1280+32*/ 1536, /*1536+8*/ 1792, 2048,
                                   /*2048+8*/ 2304, /*2304+4*/ 2560, 2560, 2560},
              2560);
    local_map(17, 17, 17, 17,
              {0, /*a256(136)*/ 256, 512, /*a256(512+64)*/ 768, /*a256(768+136)*/ 1024, /*a256(1024+816)*/ 2048,
               /*a256(2048+476)*/ 2560, /*a256(2560+17)*/ 2816, /*a256(2816+204)*/ 3072, /*a256(3072+204)*/ 3328,
               /*a256(3328+68)*/ 3584, 3840, /*a256(3840+72)*/ 4096, /*a256(4096+17)*/ 4352, /*a256(4352+68)*/ 4608},
              /*a256(4608+68)*/ 4864, /*16+40*17*/ 696,
              {/*a256(696)*/ 768, /*a256(768+17)*/ 1024, /*a256(1024+68)*/ 1280, /*a256(1280+4)*/ 1536,
               /*a256(1536+544)*/ 2304, /*a256(2304+544)*/ 3072, /*a256(3072+72)*/ 3328, /*a256(3328+4)*/ 3584,
               /*a256(3584+136)*/ 3840, /*a256(3840+68)*/ 4096, /*a256(4096+884)*/ 5120, /*a256(5120+136)*/ 5376},
              /*a256(5376+17)*/ 5632);
    // [job 88][counts 8][nl*28][nr*28][nl*32][nr*32] then [nl*4] three times
    stereo_matches(17, 0, {0, 256, 512, /*a256(512+476)*/ 1024, 1024, /*a256(1024+544)*/ 1792}, 1792,
                   {1792, /*a256(1792+68)*/ 2048, 2304}, 2560);
    stereo_matches(1, 17, {0, 256, 512, 768, /*a256(768+476)*/ 1280, /*a256(1280+32)*/ 1536}, /*a256(1536+544)*/ 2304,
                   {2304, 2560, 2816}, 3072);
    // 63 x 47 float depth image: 11844 bytes, a16 = 11856
    stereo_from_rgbd(63, 47, 17, 11856, /*11856+480*/ 12336);
    stereo_from_rgbd(63, 47, 1, 11856, /*11856+32*/ 11888);
    // N = max(n, 1): [N*32][N*4][N*8][N*4][N*4][N*8][N*4][N*4][16]
    bow_one(0, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048}, 2304);
    bow_one(17, {0, /*a256(544)*/ 768, /*a256(768+68)*/ 1024, /*a256(1024+136)*/ 1280, /*a256(1280+68)*/ 1536, 1792,
                 /*a256(1792+136)*/ 2048, 2304, 2560},
            /*a256(2560+16)*/ 2816);
    // run_match: nothing but the floors; what comes back ends with the 16 counter bytes, padded
    run_match(0, 0, false, 0, {0, 0, 0, 0, 0, 0}, 256, {0, 256, 512, 768, /*768+256*/ 1024, 1280, 1536}, 768, 1792);
    run_match(17, 17, true, 1,
              {0, /*a256(544)*/ 768, /*a256(768+544)*/ 1536, /*a256(1536+68)*/ 1792, /*a256(1792+72)*/ 2048, 2304},
              /*a256(2304+17)*/ 2560, {0, 256, 512, 768, /*768+8*32*17*/ 5120, 5376, 5632}, 768, 5888);
    // in [ptr 8][cam 16][bf 4][T 28][levels*4][rows*28][rows*12][rows*4][rows], out [result 168][rows]
    pose_optimization(0, 1, {16, 32, 48, /*48+32*/ 80, /*80+16*/ 96, /*96+32*/ 128, /*128+16*/ 144, /*144+16*/ 160},
                      /*160+16*/ 176, /*a16(168)*/ 176, /*176+16*/ 192);
    pose_optimization(17, 8, {16, 32, 48, 80, /*80+32*/ 112, /*112+480*/ 592, /*592+208*/ 800, /*800+80*/ 880},
                      /*880+32*/ 912, 176, /*176+32*/ 208);
}

// ---------------------------------------------------------------- 2. any sequence of takes
static void sequences() {
    const size_t counts[] = {0, 1, 17}, elems[] = {1, 4, 12, 28};
    for (size_t align : kAligns) {
        BlockLayout L{align};
        EXPECT(L.size(), 0);
        EXPECT(L.end(), 0);
        size_t prev_end = 0;
        // every ordered pair of (count, elem) parts follows every other once
        for (size_t a = 0; a < 12; a++)
            for (size_t b = 0; b < 12; b++)
                for (int half = 0; half < 2; half++) {
                    const size_t k = half ? b : a;
                    const size_t bytes = counts[k % 3] * elems[k / 3], before = L.size();
                    const size_t o = L.take(counts[k % 3], elems[k / 3]);
                    EXPECT(o % align, 0);
                    EXPECT(o >= prev_end, 1);       // no overlap with the part before
                    EXPECT(o, before);              // and no gap beyond its padding
                    EXPECT(L.end(), o + bytes);
                    EXPECT(L.size() >= L.end(), 1);  // the total covers the last part
                    EXPECT(L.size() - L.end() < align, 1);
                    EXPECT(L.size() % align, 0);
                    if (bytes == 0) EXPECT(L.size(), before);  // a zero-byte part takes no space
                    prev_end = o + bytes;
                }
    }
}

// ---------------------------------------------------------------- 3. write and read back
template <class T>
static void fill(uint8_t *base, size_t off, size_t count, uint8_t seed) {
    uint8_t *p = reinterpret_cast<uint8_t *>(at<T>(base, off));
    for (size_t i = 0; i < count * sizeof(T); i++) p[i] = (uint8_t)(seed + i);
}
template <class T>
static void verify(const uint8_t *base, size_t off, size_t count, uint8_t seed) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(at<T>(base, off));
    for (size_t i = 0; i < count * sizeof(T); i++) EXPECT(p[i], (uint8_t)(seed + i));
}

static void write_read_back() {
    const size_t counts[] = {0, 1, 17};
    for (size_t align : kAligns)
        for (size_t c0 : counts)
            for (size_t c1 : counts) {
                // [usable c0][int32 c1][xyz c0][kp c1][usable c1], the last part unpadded
                BlockLayout L{align};
                const size_t o_u = L.take(c0), o_i = L.take(c1, 4), o_x = L.take(c0, sizeof(Xyz));
                const size_t o_k = L.take(c1, sizeof(Kp)), o_t = L.take(c1);
                const size_t total = L.end();
                uint8_t *exact = static_cast<uint8_t *>(malloc(total ? total : 1));  // ASan guards its end
                if (!exact) { printf("allocation failed\n"); exit(2); }
                fill<uint8_t>(exact, o_u, c0, 1);
                fill<int32_t>(exact, o_i, c1, 2);
                fill<Xyz>(exact, o_x, c0, 3);
                fill<Kp>(exact, o_k, c1, 4);
                fill<uint8_t>(exact, o_t, c1, 5);
                verify<uint8_t>(exact, o_u, c0, 1);
                verify<int32_t>(exact, o_i, c1, 2);
                verify<Xyz>(exact, o_x, c0, 3);
                verify<Kp>(exact, o_k, c1, 4);
                verify<uint8_t>(exact, o_t, c1, 5);
                // typed access: the first int32 and the last keypoint of their parts
                if (c1) {
                    *at<int32_t>(exact, o_i) = -7;
                    at<Kp>(exact, o_k)[c1 - 1].i[1] = 9;
                    const uint8_t *ro = exact;
                    EXPECT((size_t)(*at<int32_t>(ro, o_i) == -7), 1);
                    EXPECT((size_t)at<Kp>(ro, o_k)[c1 - 1].i[1], 9);
                }
                free(exact);
            }
}

int main() {
    reference_layouts();
    sequences();
    write_read_back();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("staging layout ok\n");
    return 0;
}
