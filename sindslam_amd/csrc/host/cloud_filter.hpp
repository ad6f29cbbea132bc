// Statistical outlier filter of the key-frame cloud (reference octomap_pub/src/pubPointCloud.cc:291-296: pcl::StatisticalOutlierRemoval, setMeanK(100),
// setStddevMulThresh(1.0)), restated from PCL 1.10's StatisticalOutlierRemoval<PointT>::applyFilterIndices over KdTreeFLANN with flann::L2_Simple<float>.
// Parity with a real PCL / FLANN build is UNPINNED (neither is available to this project); the contract below is what the kernels (csrc/cloud_filter.hip), the host
// twin (csrc/host/cloud_filter.cpp) and tests/cloud_filter_ref.py agree on, bit for bit.  ONE source for the arithmetic of host and device: the squared distance, the
// ordered FP64 sum, the statistics and the verdict.  The neighbour SEARCH is not here: the device and the twin each have their own, so that they check each other.
//   finite point       x, y, z all finite; only finite points are neighbours; a non-finite point gets distance 0 and is not counted in valid
//   squared distance   FP32, uncontracted: d = 0; d += dx*dx; d += dy*dy; d += dz*dz
//   mean distance      the mean_k + 1 smallest squared distances over all finite j (j == i included), ascending, the first dropped; sum (FP64, from 0) of
//                      sqrt((double)d) in ascending order; distance = (float)(sum / mean_k).  A function of the multiset: ties cannot change it.
//   statistics         sum += d, sq_sum += (double)(d * d) (FP32 product) over ALL points in index order; mean = sum / valid;
//                      variance = (sq_sum - sum * sum / valid) / (valid - 1.0); stddev = sqrt(variance); threshold = mean + stddev_mul * stddev, taken literally: a
//                      slightly negative variance gives a NaN (reported with the bits 0x7ff8000000000000 in stddev and threshold, whatever the processor made)
//   verdict            removed iff distance > threshold (so nothing is removed under a NaN threshold, and non-finite points stay)
//   fewer than mean_k + 1 finite points: the reference reads past its neighbour arrays; here the cloud is kept unchanged, degenerate = 1, threshold = mean =
//                      stddev = 0, all distances 0 -- the one deliberate divergence.
#pragma once
#include <cmath>
#include <cstdint>
#include "peac_fit.hpp"                                              // SIND_HD

namespace sind {

constexpr int CF_MAX_MEAN_K = 128;                                   // the built maximum of mean_k

SIND_HD inline bool cf_finite(float x, float y, float z) {           // bit test: the same on both sides whatever the fast-math state of a translation unit
    union { float f; uint32_t u; } a, b, c; a.f = x; b.f = y; c.f = z;
    return (a.u & 0x7f800000u) != 0x7f800000u && (b.u & 0x7f800000u) != 0x7f800000u && (c.u & 0x7f800000u) != 0x7f800000u;
}
SIND_HD inline float cf_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float d = 0.0f; d += dx * dx; d += dy * dy; d += dz * dz;
    return d;
}
SIND_HD inline double cf_root(float d2) { return sqrt((double)d2); }
// root(i), i = 0 .. mean_k - 1: the roots of the neighbours' squared distances in ascending order (the query itself already dropped)
template <class Root> SIND_HD inline float cf_mean_distance(Root root, int mean_k) {
    double sum = 0.0;
    for (int i = 0; i < mean_k; i++) sum += root(i);
    return (float)(sum / mean_k);
}
// the sign and payload of a NaN are the processor's choice (x86 sets the sign bit on the sqrt of a negative; nothing obliges a GPU to): a NaN is reported as 0x7ff8000000000000
SIND_HD inline double cf_canonical(double v) {
    union { double d; uint64_t u; } c; c.d = v;
    if ((c.u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) c.u = 0x7ff8000000000000ull;
    return c.d;
}
struct CfAcc { double sum = 0.0, sq = 0.0; SIND_HD void add(float d) { sum += d; sq += (double)(d * d); } };
struct CfMoments { double mean, stddev, threshold; };
SIND_HD inline CfMoments cf_moments(const CfAcc& a, int valid, double stddev_mul) {
    CfMoments m;
    m.mean = a.sum / (double)valid;
    const double variance = (a.sq - a.sum * a.sum / (double)valid) / ((double)valid - 1.0);
    m.stddev = cf_canonical(sqrt(variance));
    m.threshold = cf_canonical(m.mean + stddev_mul * m.stddev);
    return m;
}
SIND_HD inline bool cf_removed(float distance, double threshold) { return (double)distance > threshold; }

}  // namespace sind
