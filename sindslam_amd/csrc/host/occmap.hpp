// Occupancy map of the mapping consumer (reference octomap_pub/src/pubPointCloud.cc:299-365: octomap::ColorOcTree::insertRay per point, integrateNodeColor per point,
// the walk over the occupied leaves), restated from octomap 1.9 as recalled: OcTreeBaseImpl::coordToKeyChecked / keyToCoord / computeRayKeys, OccupancyOcTreeBase::
// insertRay / updateNodeLogOdds, ColorOcTree::integrateNodeColor.  Parity with a real octomap build is UNPINNED (octomap is not available to this project); the contract
// in include/sind_hip.h ("sind_occmap_*") is what the kernels (csrc/occmap_kernels.hip), the host twin (csrc/host/occmap.cpp) and tests/occmap_ref.py agree on, bit for
// bit.  ONE source for the arithmetic of host and device: the key of a coordinate, the DDA's initialisation and step, the log-odds update, a run of equal updates and
// the colour blend.  The SCHEDULE is not here: the twin runs the literal sequential loops, the device counts and replays (see occmap_kernels.hip).
//   The map is flat: every voxel lives at depth 16, no pruning.  Non-finite coordinates never reach these functions (the callers skip them).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include "fd_exp.hpp"

namespace sind {

constexpr int OCC_KEY_OFFSET = 32768, OCC_KEY_RANGE = 65536;
constexpr uint64_t OCC_EMPTY = ~0ull;                                // no packed key has its upper 16 bits set

struct OccParams { double res, resFactor; float hitLog, missLog, clampMinLog, clampMaxLog, occLog; };

// (float) log(p / (1 - p)), once, on the host, with the C library; never on the device
inline float occ_logodds(double p) { return (float)std::log(p / (1.0 - p)); }
inline OccParams occ_params(double res, double hit, double miss, double cmin, double cmax, double occ) {
    return OccParams{res, 1.0 / res, occ_logodds(hit), occ_logodds(miss), occ_logodds(cmin), occ_logodds(cmax), occ_logodds(occ)};
}

SIND_HD inline bool occ_finite(float x, float y, float z) {          // bit test, as cf_finite: the same whatever the fast-math state of a translation unit
    union { float f; uint32_t u; } a, b, c; a.f = x; b.f = y; c.f = z;
    return (a.u & 0x7f800000u) != 0x7f800000u && (b.u & 0x7f800000u) != 0x7f800000u && (c.u & 0x7f800000u) != 0x7f800000u;
}
// key(c) = (int) floor(resFactor * (double) c) + 32768, valid iff 0 <= key < 65536.  The range is tested on the floor itself, so that no cast overflows.
SIND_HD inline bool occ_key(const OccParams& P, float c, int* k) {
    const double f = floor(P.resFactor * (double)c);
    if (!(f >= -(double)OCC_KEY_OFFSET && f < (double)OCC_KEY_OFFSET)) return false;
    *k = (int)f + OCC_KEY_OFFSET; return true;
}
SIND_HD inline bool occ_key3(const OccParams& P, float x, float y, float z, int k[3]) {
    const bool a = occ_key(P, x, k), b = occ_key(P, y, k + 1), c = occ_key(P, z, k + 2);
    return a && b && c;
}
SIND_HD inline double occ_coord(const OccParams& P, int k) { return ((double)(k - OCC_KEY_OFFSET) + 0.5) * P.res; }
SIND_HD inline uint64_t occ_pack(const int k[3]) { return (uint64_t)k[0] | ((uint64_t)k[1] << 16) | ((uint64_t)k[2] << 32); }
SIND_HD inline uint64_t occ_pack(int x, int y, int z) { return (uint64_t)x | ((uint64_t)y << 16) | ((uint64_t)z << 32); }

// computeRayKeys.  Scalars per axis, not arrays: the device must not index registers dynamically.
struct OccRay { int k0, k1, k2, e0, e1, e2, s0, s1, s2; double t0, t1, t2, d0, d1, d2, length; };

SIND_HD inline void occ_axis(const OccParams& P, int key, float origin, float dir, int* step, double* tMax, double* tDelta) {
    *step = dir > 0.0f ? 1 : dir < 0.0f ? -1 : 0;                    // a NaN direction (a ray shorter than FP32 can square) does not step
    if (*step != 0) {
        const double border = occ_coord(P, key) + (double)(float)(*step * P.res * 0.5);
        *tMax = (border - (double)origin) / (double)dir;
        *tDelta = P.res / fabs((double)dir);
    } else { *tMax = DBL_MAX; *tDelta = DBL_MAX; }
}
// the keys differ; the miss list starts with ko itself (the caller appends it), then every key for which occ_ray_step returns true
SIND_HD inline void occ_ray_init(const OccParams& P, const float o[3], const float e[3], const int ko[3], const int ke[3], OccRay& r) {
    float dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
    float sum = dx * dx; sum = sum + dy * dy; sum = sum + dz * dz;
    const float length = sqrtf(sum);
    dx = dx / length; dy = dy / length; dz = dz / length;
    r.k0 = ko[0]; r.k1 = ko[1]; r.k2 = ko[2]; r.e0 = ke[0]; r.e1 = ke[1]; r.e2 = ke[2]; r.length = (double)length;
    occ_axis(P, ko[0], o[0], dx, &r.s0, &r.t0, &r.d0); occ_axis(P, ko[1], o[1], dy, &r.s1, &r.t1, &r.d1); occ_axis(P, ko[2], o[2], dz, &r.s2, &r.t2, &r.d2);
}
// One turn of the loop.  true: (k0, k1, k2) is the next key of the miss list; false: the loop has ended (the end key reached, or every tMax beyond the length).
// The guard is not octomap's: a key that would leave [0, 65536) ends the ray (only a ray whose FP32 length underflows to 0 gets there; octomap's loop never ends on it).
SIND_HD inline bool occ_ray_step(OccRay& r) {
    const int dim = r.t0 < r.t1 ? (r.t0 < r.t2 ? 0 : 2) : (r.t1 < r.t2 ? 1 : 2);      // strict: a tie goes to the later axis
    int moved;
    if (dim == 0) { r.k0 += r.s0; r.t0 += r.d0; moved = r.k0; } else if (dim == 1) { r.k1 += r.s1; r.t1 += r.d1; moved = r.k1; } else { r.k2 += r.s2; r.t2 += r.d2; moved = r.k2; }
    if (moved < 0 || moved >= OCC_KEY_RANGE) return false;
    if (r.k0 == r.e0 && r.k1 == r.e1 && r.k2 == r.e2) return false;
    const double m01 = r.t0 < r.t1 ? r.t0 : r.t1, m = m01 < r.t2 ? m01 : r.t2;
    if (m > r.length) return false;
    return true;
}

// A voxel's value.  known = 0: nothing else is meaningful.
struct OccVoxel { float v; uint8_t r, g, b, known; };
SIND_HD inline void occ_make_known(OccVoxel& x) { if (!x.known) { x.known = 1; x.v = 0.0f; x.r = x.g = x.b = 255; } }
SIND_HD inline float occ_clamped_add(const OccParams& P, float v, float u) {
    float w = v + u;
    if (w < P.clampMinLog) w = P.clampMinLog;
    if (w > P.clampMaxLog) w = P.clampMaxLog;
    return w;
}
SIND_HD inline void occ_update(const OccParams& P, OccVoxel& x, float u) { occ_make_known(x); x.v = occ_clamped_add(P, x.v, u); }
// n times occ_update(u): the value is a function of the previous one, so once it stops changing it never changes again (at most ~14 turns separate the clamps)
SIND_HD inline void occ_update_run(const OccParams& P, OccVoxel& x, float u, int n) {
    if (n <= 0) return;
    occ_make_known(x);
    for (int i = 0; i < n; i++) { const float w = occ_clamped_add(P, x.v, u); if (w == x.v) break; x.v = w; }
}
// integrateNodeColor on a known voxel: (255, 255, 255) is "not set" and takes the colour; otherwise the blend by the node's occupancy probability
SIND_HD inline double occ_probability(float logodds) { return 1. - (1. / (1. + s3_exp((double)logodds))); }
SIND_HD inline uint8_t occ_blend(uint8_t prev, uint8_t now, double p) { return (uint8_t)((double)prev * p + (double)now * (0.99 - p)); }
SIND_HD inline void occ_colour(OccVoxel& x, uint8_t r, uint8_t g, uint8_t b, double p) {
    if (x.r == 255 && x.g == 255 && x.b == 255) { x.r = r; x.g = g; x.b = b; return; }
    x.r = occ_blend(x.r, r, p); x.g = occ_blend(x.g, g, p); x.b = occ_blend(x.b, b, p);
}

// leaf_iterator order: ascending Morton code of the key from bit 15 down, z the most significant bit of each triple, then y, then x
inline uint64_t occ_morton(uint64_t packed) {
    uint64_t m = 0;
    for (int b = 15; b >= 0; b--) m = (m << 3) | (((packed >> (32 + b)) & 1) << 2) | (((packed >> (16 + b)) & 1) << 1) | ((packed >> b) & 1);
    return m;
}

}  // namespace sind
