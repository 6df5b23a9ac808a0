// api_hamming.cpp — brute-force Hamming matching: device and host entry points, the batch's pairs.
#include <string.h>

#include "host.hpp"

extern "C" {

// ------------------------------------------------------------------ hamming
int ygzfe_hamming_best2_device(const uint8_t *d_query, int nq, const uint8_t *d_train, int nt, int32_t *d_best_idx,
                               int32_t *d_best_dist, int32_t *d_second_dist, void *stream) {
    if (nq < 0 || nt < 0 || (nq > 0 && (!d_query || !d_best_idx || !d_best_dist || !d_second_dist)) ||
        (nt > 0 && !d_train)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    YGZ_HIP(launch_hamming_best2(d_query, nq, d_train, nt, d_best_idx, d_best_dist, d_second_dist,
                                 (hipStream_t)stream));
    return YGZFE_OK;
}

int ygzfe_hamming_best2(int device, const uint8_t *query, int nq, const uint8_t *train, int nt, int32_t *best_idx,
                        int32_t *best_dist, int32_t *second_dist) {
    if (nq < 0 || nt < 0 || (nq > 0 && (!query || !best_idx || !best_dist || !second_dist)) || (nt > 0 && !train)) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (nq == 0) return YGZFE_OK;
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    BlockLayout in{16};  // in: [query][train]  out: [best_idx][best_dist][second_dist]
    const size_t o_q = in.take(nq, 32), o_t = in.take(nt > 0 ? nt : 1, 32), in_bytes = in.size();
    const size_t out_bytes = (size_t)nq * 12;
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>();
    memcpy(h + o_q, query, (size_t)nq * 32);
    if (nt > 0) memcpy(h + o_t, train, (size_t)nt * 32);
    YGZ_TRY(S.upload(in_bytes));
    int32_t *bi = at<int32_t>(d, in_bytes), *bd = bi + nq, *sd = bd + nq;
    YGZ_HIP(launch_hamming_best2(d + o_q, nq, d + o_t, nt, bi, bd, sd, S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    const int32_t *ho = S->hout.as<int32_t>();
    memcpy(best_idx, ho, (size_t)nq * 4);
    memcpy(best_dist, ho + nq, (size_t)nq * 4);
    memcpy(second_dist, ho + 2 * (size_t)nq, (size_t)nq * 4);
    return YGZFE_OK;
}

int ygzfe_hamming_csr(int device, const uint8_t *query, int nq, const uint8_t *train, int nt, const int32_t *row_ptr,
                      const int32_t *cand, int32_t *dist_out) {
    if (nq < 0 || nt < 0 || !row_ptr) { set_error("invalid argument"); return YGZFE_EINVAL; }
    if (nq == 0) return YGZFE_OK;
    const int nc = row_ptr[nq];
    if (nc == 0) return YGZFE_OK;
    if (!query || !train || !cand || !dist_out) { set_error("invalid argument"); return YGZFE_EINVAL; }
    for (int k = 0; k < nc; k++)
        if (cand[k] < 0 || cand[k] >= nt) { set_error("candidate index %d out of range", cand[k]); return YGZFE_EINVAL; }
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    BlockLayout in{16};  // in: [query][train][row_ptr][cand]  out: [dist]
    const size_t o_q = in.take(nq, 32), o_t = in.take(nt, 32), o_r = in.take((size_t)nq + 1, 4), o_c = in.take(nc, 4);
    const size_t in_bytes = in.size(), out_bytes = (size_t)nc * 4;
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>();
    memcpy(h + o_q, query, (size_t)nq * 32);
    memcpy(h + o_t, train, (size_t)nt * 32);
    memcpy(h + o_r, row_ptr, (size_t)(nq + 1) * 4);
    memcpy(h + o_c, cand, (size_t)nc * 4);
    YGZ_TRY(S.upload(in_bytes));
    YGZ_HIP(launch_hamming_csr(d + o_q, nq, d + o_t, at<const int32_t>(d, o_r), at<const int32_t>(d, o_c),
                               at<int32_t>(d, in_bytes), S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    memcpy(dist_out, S->hout.p, out_bytes);
    return YGZFE_OK;
}

int ygzfe_batch_match(ygzfe_batch *b, int n_pairs, const int32_t *d_qframe, const int32_t *d_tframe,
                      int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_second_dist, void *stream) {
    if (!b || n_pairs < 0) { set_error("invalid argument"); return YGZFE_EINVAL; }
    YGZ_TRY(ensure_device(b->device));
    hipStream_t st = stream ? (hipStream_t)stream : b->stream;
    const Plan &P = b->plan->hp();
    hipEvent_t t0 = b->begin(st);
    YGZ_HIP(launch_hamming_best2_pairs(b->ws.desc.as<uint8_t>(), b->ws.counts.as<int32_t>(), P.kp_cap, n_pairs,
                                       d_qframe, d_tframe, d_best_idx, d_best_dist, d_second_dist, st));
    b->end(ST_HAM, t0, st);
    return YGZFE_OK;
}

}  // extern "C"
