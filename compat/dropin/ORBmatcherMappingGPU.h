// ORBmatcherMappingGPU.h — the mapping-side ORBmatcher search on the GPU, read through the
// reference's own KeyFrame members.
//
//   SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, Matrix3f &F12, vMatchedPairs, bOnlyStereo)
//                                                                          ORBmatcher.cc:597-746
// ORBmatcher.cc includes ORBmatcher_mapping_gpu.inc in place of that body, so
// LocalMapping::CreateNewMapPoints (LocalMapping.cc:1042) compiles and runs unchanged: one device
// call per neighbour.  gpu::SearchForTriangulationAll searches every neighbour in ONE call
// (ygzfe_search_for_triangulation_batch): CreateNewMapPoints first collects the neighbours that pass
// its baseline test with their F12, calls it once, and its loop then takes vMatchedIndices from the
// result.
//
// Gathered here on the host with the caller's matrix types, exactly as the reference forms them:
// GetMapPoint(i) != NULL per keypoint, the two FeatureVectors as CSR, the epipole (:603-609).  The
// node walk's candidates, Hamming distances, the epipolar tests, the tie rule and the rotation check
// run on the GPU.  The keyframes' mvKeys / mDescriptors / mvuRight stay on the device between calls:
// a view whose content is byte-equal to its last upload is not uploaded again (neighbours repeat
// from one new keyframe to the next).
#ifndef YGZFE_ORBMATCHER_MAPPING_GPU_H_
#define YGZFE_ORBMATCHER_MAPPING_GPU_H_

#include <algorithm>
#include <utility>
#include <vector>

#include "ORBmatcherGPU.h"

namespace ygz {
namespace gpu {

// the views of one mapping thread: [0] the new keyframe, [1 + k] neighbour k
inline MatchView &mapping_view(size_t slot) {
    static thread_local std::vector<MatchView *> v;  // kept for the thread's lifetime
    while (v.size() <= slot) v.push_back(new MatchView((int)v.size()));
    return *v[slot];
}

template <class KeyFrameT>
inline bool set_keyframe(MatchView &v, KeyFrameT *pKF) {
    const int n = pKF->N;
    // this search reads no grid: any non-empty bounds do
    const ygzfe_bounds b = {0.f, 1.f, 0.f, 1.f};
    return v.set(pKF->mvKeys, pKF->mDescriptors, n,
                 (int)pKF->mvuRight.size() >= n && n > 0 ? pKF->mvuRight.data() : nullptr, b);
}

// SearchForTriangulation(pKF1, vpKF2[k], vF12[k], vvMatchedPairs[k], bOnlyStereo) for every k, one device
// call.  Returns the nmatches of each (the reference's return values).  mvLevelSigma2 / mvScaleFactors are
// those of the first neighbour: every keyframe of a map shares the extractor's pyramid.
template <class KeyFrameT>
std::vector<int> SearchForTriangulationAll(KeyFrameT *pKF1, const std::vector<KeyFrameT *> &vpKF2,
                                           const std::vector<Matrix3f> &vF12, const bool bOnlyStereo,
                                           std::vector<std::vector<std::pair<size_t, size_t> > > &vvMatchedPairs,
                                           const bool checkOri = false) {
    const int nnb = (int)vpKF2.size(), n1 = pKF1->N;
    vvMatchedPairs.assign(nnb, std::vector<std::pair<size_t, size_t> >());
    std::vector<int> nmatches(nnb, 0);
    if (nnb == 0 || vF12.size() != vpKF2.size()) return nmatches;
    // FeatureVectors (std::map<NodeId, std::vector<unsigned>>) as node-sorted CSR, appended
    auto csr = [](const decltype(pKF1->mFeatVec) &fv, std::vector<int32_t> &nodes, std::vector<int32_t> &ptr,
                  std::vector<int32_t> &feats) {
        for (auto it = fv.begin(); it != fv.end(); ++it) {
            nodes.push_back((int32_t)it->first);
            for (size_t k = 0; k < it->second.size(); k++) feats.push_back((int32_t)it->second[k]);
            ptr.push_back((int32_t)feats.size());
        }
    };
    std::vector<uint8_t> mp1((size_t)n1 + 1, 0), mp2;
    for (int i = 0; i < n1; i++) mp1[i] = pKF1->GetMapPoint(i) != NULL;  // :635-639
    std::vector<int32_t> n1v, p1v(1, 0), f1v, n2v, p2v(1, 0), f2v, mp2_ptr(1, 0), fv2_ptr(1, 0);
    csr(pKF1->mFeatVec, n1v, p1v, f1v);
    std::vector<ygzfe_match_frame *> frames(nnb);
    std::vector<float> F(9 * (size_t)nnb), ep(2 * (size_t)nnb);
    if (!set_keyframe(mapping_view(0), pKF1)) return nmatches;
    const Vector3f Cw = pKF1->GetCameraCenter();
    for (int k = 0; k < nnb; k++) {
        KeyFrameT *pKF2 = vpKF2[k];
        if (!set_keyframe(mapping_view(1 + k), pKF2)) return nmatches;
        frames[k] = mapping_view(1 + k).get();
        for (int i = 0; i < pKF2->N; i++) mp2.push_back(pKF2->GetMapPoint(i) != NULL);  // :657-661
        mp2_ptr.push_back(mp2_ptr.back() + pKF2->N);
        csr(pKF2->mFeatVec, n2v, p2v, f2v);
        fv2_ptr.push_back((int32_t)n2v.size());
        // :603-609, the epipole in the second image
        const Matrix3f R2w = pKF2->GetRotation();
        const Vector3f t2w = pKF2->GetTranslation();
        const Vector3f C2 = R2w * Cw + t2w;
        const float invz = 1.0f / C2[2];
        ep[2 * k] = pKF2->fx * C2[0] * invz + pKF2->cx;
        ep[2 * k + 1] = pKF2->fy * C2[1] * invz + pKF2->cy;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) F[9 * (size_t)k + 3 * r + c] = vF12[k](r, c);
    }
    const std::vector<float> &sigma2 = vpKF2[0]->mvLevelSigma2, &scale = vpKF2[0]->mvScaleFactors;
    const int nl = (int)std::min(sigma2.size(), scale.size());
    std::vector<int32_t> m12((size_t)nnb * n1 + 1);
    if (ygzfe_search_for_triangulation_batch(mapping_view(0).get(), mp1.data(), (int)n1v.size(), n1v.data(), p1v.data(),
                                             f1v.data(), nnb, frames.data(), mp2_ptr.data(), mp2.data(),
                                             fv2_ptr.data(), n2v.data(), p2v.data(), f2v.data(), F.data(), ep.data(),
                                             sigma2.data(), scale.data(), nl, bOnlyStereo ? 1 : 0, checkOri ? 1 : 0,
                                             m12.data(), nmatches.data()) != YGZFE_OK) {
        failed("SearchForTriangulation");
        return std::vector<int>(nnb, 0);
    }
    for (int k = 0; k < nnb; k++) {  // :736-743, ascending idx1
        vvMatchedPairs[k].reserve(nmatches[k]);
        for (int i = 0; i < n1; i++)
            if (m12[(size_t)k * n1 + i] >= 0)
                vvMatchedPairs[k].push_back(std::make_pair((size_t)i, (size_t)m12[(size_t)k * n1 + i]));
    }
    return nmatches;
}

// the reference's signature: one neighbour
template <class KeyFrameT>
int SearchForTriangulation(KeyFrameT *pKF1, KeyFrameT *pKF2, const Matrix3f &F12,
                           std::vector<std::pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo,
                           const bool checkOri) {
    std::vector<std::vector<std::pair<size_t, size_t> > > all;
    const std::vector<int> n = SearchForTriangulationAll(pKF1, std::vector<KeyFrameT *>(1, pKF2),
                                                         std::vector<Matrix3f>(1, F12), bOnlyStereo, all, checkOri);
    vMatchedPairs.swap(all[0]);
    return n[0];
}

}  // namespace gpu
}  // namespace ygz

#endif
