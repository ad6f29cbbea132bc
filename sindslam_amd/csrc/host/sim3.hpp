// Host half of Sim3Solver (reference src/Sim3Solver.cc): the closed-form hypothesis of one sampled triple and the constructor's per-correspondence
// arithmetic.  Plain C++, no device code: compiled into libsind_hip.so (capi_match_ransac.cpp calls it) and into libsind_host.so (sindh_sim3_horn, for the CPU tests).
#pragma once
#include <cstddef>

namespace sind {

struct Sim3Hyp { float R12[9], t12[3], s12, T12[16], T21[16]; };   // mR12i, mt12i, ms12i, mT12i, mT21i (row-major)

// Sim3Solver::ComputeSim3 (:226-337).  P1, P2: 3x3 row-major, column i = the i-th sampled point in camera 1 / camera 2 (P3Dc1i, P3Dc2i)
void sim3_horn(const float* P1, const float* P2, bool fixScale, Sim3Hyp& h);

// Rcw * X + tcw of the constructor (:95, :98) and of Project (:396); T = rows 0..2 of a row-major 4x4
inline void sim3_to_camera(const float* T, const float* X, float* xc) {
    for (int r = 0; r < 3; r++) { const float t = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2]; xc[r] = (float)((double)t * 1.0 + (double)T[4 * r + 3] * 1.0); }
}
// FromCameraToImage (:405-423)
inline void sim3_to_image(float fx, float fy, float cx, float cy, const float* xc, float* uv) {
    const float invz = 1 / xc[2], x = xc[0] * invz, y = xc[1] * invz;
    uv[0] = fx * x + cx; uv[1] = fy * y + cy;
}
// mvnMaxError1/2 (:87-88, include/Sim3Solver.h:78-79): a size_t, as the float that `err < bound` compares with.  sigma2 >= 0 and finite (the caller checks)
inline float sim3_max_error(float sigma2) { return (float)(size_t)(9.210 * sigma2); }

}  // namespace sind
