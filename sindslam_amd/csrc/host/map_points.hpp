// The arithmetic on the map points themselves: the per-match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:284-431, with
// KeyFrame::UnprojectStereo, src/KeyFrame.cc:615-631) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:330-371).  ONE source for the host (map_points.cpp:
// sindh_triangulate, sindh_update_points) and the device (../match_mappoints.hip: k_tri_points, k_mp_normal), as epnp.hpp is: IEEE add / mul / div / sqrt in
// FP32 and FP64 on both sides and no contraction (-ffp-contract=off), so the two give the same bits.  No libm / ocml call besides sqrt and fabs: hypot is
// DEFINED here (mp_hypot, the scaled-sqrt form of OpenCV's lapack.cpp, as epnp_hypot).  MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) is
// integer work: the host twin transcribes it literally (all-pairs distances, std::sort, the median; map_points.cpp), the device finds the same median by
// bisection (k_mp_descriptor), and the two are compared.
//
// PARITY WITH A REAL OPENCV BUILD IS UNPINNED, as for every restated primitive: OpenCV is not available to build or run, so each one is restated from OpenCV
// 4.2.0 as remembered.  tests/mappoints_ref.py is the same restatement in Python (bit equality BY CONSTRUCTION); tests/test_mappoints_cpu.py also compares the
// triangulated points with an FP64 LAPACK solution of the same A, which shares none of the guesses.  The conventions are (1)-(7) at the head of
// ../match_local.hip; the line-by-line types of the loop:
//   xn = ((x - cx) * invfx, (y - cy) * invfy, 1)     FP32, invfx = 1.0f / fx as Frame.cc forms it
//   ray = Rwc * xn                                  Rwc = Rcw.t() of Tcw; FP32 row product (a0 b0 + a1 b1) + a2 b2                                       (1)
//   cosParallaxRays                                 (float)(dot / (norm1 * norm2)): Mat::dot and cv::norm return double, FP64 accumulation in order       (3) (4)
//   cos(2 * atan2(mb / 2, depth))                   the FLOAT overloads: DBoW2's TemplatedVocabulary.h (included through ORBVocabulary.h by KeyFrame.h) has
//                                                   `using namespace std;` at global scope and both arguments are float, so the call is std::atan2(float, float)
//                                                   and std::cos(float); mb = bf / fx in FP32.  NEVER evaluated on the device: the entry points evaluate it on
//                                                   the host with the C library (atan2f, cosf), once per match with a stereo side, as the Sim3 solver does for
//                                                   its atan2, sin and cos; TriMatch carries the result.  Only the one cosine the reference evaluates is formed
//                                                   (`if (bStereo1) .. else if (bStereo2)`: a match that is stereo on both sides never gets cosParallaxStereo2)
//   min(c1, c2)                                     std::min: c2 < c1 ? c2 : c1
//   cosParallaxRays < 0.9998                        the float promoted to double
//   A.row(k) = x * T.row(2) - T.row(r)              every element T2 * (float)x - Tr in FP32                                                              (5)
//   cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV)   m = n = 4: At = A^T, JacobiSVDImpl_<float>(At, w, Vt, 4, 4, 4) with minval = FLT_MIN and
//                                                   eps = FLT_EPSILON * 2, vt = Vt.  The float instance keeps W, the dot product p, beta, gamma and delta in
//                                                   double and c, s and the rotated elements in float; sweep order, thresholds and the descending selection sort
//                                                   as epnp_jacobi_svd.  Its tail for zero singular values (the fill-in generator) rewrites rows of At alone,
//                                                   that is of u, which the reference never reads: it is skipped, as epnp.hpp skips Vt where no caller reads it.
//                                                   x3D = row 3 of vt                                                                    [G: that VBLAS<float>::givens rounds as the scalar loop]
//   x3D.rowRange(0, 3) / x3D(3)                     every element times (float)(1.0 / (double)w) in FP32                                                  (5)
//   UnprojectStereo                                 x = (u - cx) * z * invfx, left to right in FP32, u v = the DISTORTED key (mvKeys); Rwc x3Dc + twc of Twc:
//                                                   FP32 row product, then (float)((double)t + (double)twc[r])                                            (1)
//   z = Rcw.row(2).dot(x3Dt) + tcw(2)               (float)(dot + (double)tcw(2)), dot in FP64; x, y likewise                                             (4)
//   invz = 1.0 / z                                  (float)(1.0 / (double)z)
//   err > 5.991 * sigmaSquare, 7.8 * sigmaSquare    FP32 sum of squares promoted, against the double product; mvLevelSigma2[l] = scale[l] * scale[l] in FP32
//   u_r = u - mbf * invz                            key frame 2's test uses the CURRENT key frame's mbf, as written; one handle holds one bf anyway
//   dist = cv::norm(x3D - Ow)                       FP32 difference, squares summed in FP64, (float)sqrt; Ow = column 3 of Twc                            (3)
//   ratioFactor                                     1.5f * scale[1]
// and of UpdateNormalAndDepth:
//   normal = normal + normali / cv::norm(normali)   normali * (float)(1.0 / norm) + normal in FP32 (cv::scaleAdd), sequential in list order, bad key frames included   (5)
//   dist, mfMaxDistance, mfMinDistance              (3); dist * scale[level]; mfMaxDistance / scale[nlevels - 1] in FP32
//   mNormalVector = normal / n                      every element times (float)(1.0 / (double)n)                                                          (5)
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>
#include "peac_fit.hpp"                                              // SIND_HD

struct sind_tri_pair;
struct sind_mappoints_item;

// LIMITS of one item of sind_match_update_points (beyond them SIND_E_CAPACITY): local BA's
#define MPU_MAX_KF 4096
#define MPU_MAX_MP 65536
#define MPU_MAX_OBS (1 << 20)

namespace sind {

struct TriCam { float fx, fy, cx, cy, invfx, invfy, bf, ratioFactor; float scale[16], sigma2[16]; };
struct TriPair { float Tcw1[12], Twc1[12], Tcw2[12], Twc2[12]; };   // rows 0..2 of GetPose() and GetPoseInverse() of the current key frame and of the neighbour
struct TriMatch {                                                   // one entry of vMatchedIndices with what the loop reads of its two keypoints
    float un1[2], xy1[2], ur1, depth1, cos1; int oct1;               // cos1: cosParallaxStereo1 where bStereo1, else unused
    float un2[2], xy2[2], ur2, depth2, cos2; int oct2;               // cos2: cosParallaxStereo2 where bStereo2 and not bStereo1, else unused
    int pair, idx1;
};
struct TriOut { float x3D[3]; int how, status; };
enum { TRI_NEW = 0, TRI_LOW_PARALLAX = 1, TRI_W0 = 2, TRI_Z1 = 3, TRI_Z2 = 4, TRI_REPROJ1 = 5, TRI_REPROJ2 = 6, TRI_DIST0 = 7, TRI_SCALE = 8 };

SIND_HD inline double mp_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

SIND_HD inline double mp_dot3(const float* a, const float* b) { double s = 0; for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k]; return s; }
SIND_HD inline double mp_norm3(const float* a) { return sqrt(mp_dot3(a, a)); }

// one Jacobi rotation of rows i and j (of At with its squared norms wi, wj, and of Vt) -> whether it rotated
SIND_HD inline bool mp_jacobi_pair(float* Ai, float* Aj, float* Vi, float* Vj, double& wi, double& wj) {
    const float eps = FLT_EPSILON * 2;
    double a = wi, p = 0, b = wj;
    for (int k = 0; k < 4; k++) p += (double)Ai[k] * (double)Aj[k];
    if (fabs(p) <= (double)eps * sqrt(a * b)) return false;
    p *= 2;
    const double beta = a - b, gamma = mp_hypot(p, beta);
    float c, s;
    if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)sqrt(delta / gamma); c = (float)(p / (gamma * (double)s * 2)); }
    else { c = (float)sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * (double)c * 2)); }
    a = b = 0;
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
        Ai[k] = t0; Aj[k] = t1;
        a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
    }
    wi = a; wj = b;
    for (int k = 0; k < 4; k++) { const float t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
    return true;
}

// JacobiSVDImpl_<float>(At, W, Vt, 4, 4, 4) up to the sort: At [4][4] holds A^T on entry; x = row 3 of Vt after the descending sort.  Every index below is a
// constant after unrolling, so the 32 floats and 4 doubles of a match stay in registers on the device.
SIND_HD inline void mp_svd4_last_row(float At[4][4], float x[4]) {
    float Vt[4][4]; double W[4];
    for (int i = 0; i < 4; i++) {
        double sd = 0;
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * (double)t; Vt[i][k] = i == k ? 1.0f : 0.0f; }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; iter++) {                           // max_iter = max(m, 30)
        bool changed = false;
        changed |= mp_jacobi_pair(At[0], At[1], Vt[0], Vt[1], W[0], W[1]);
        changed |= mp_jacobi_pair(At[0], At[2], Vt[0], Vt[2], W[0], W[2]);
        changed |= mp_jacobi_pair(At[0], At[3], Vt[0], Vt[3], W[0], W[3]);
        changed |= mp_jacobi_pair(At[1], At[2], Vt[1], Vt[2], W[1], W[2]);
        changed |= mp_jacobi_pair(At[1], At[3], Vt[1], Vt[3], W[1], W[3]);
        changed |= mp_jacobi_pair(At[2], At[3], Vt[2], Vt[3], W[2], W[3]);
        if (!changed) break;
    }
    for (int i = 0; i < 4; i++) {
        double sd = 0;
        for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * (double)t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < 3; i++) {                                     // selection sort, descending: j = the first index of the largest of W[i..3]
        int j = i; double wj = W[i];
        for (int k = i + 1; k < 4; k++) if (wj < W[k]) { j = k; wj = W[k]; }
        for (int k = i + 1; k < 4; k++) if (j == k) {
            const double t = W[i]; W[i] = W[k]; W[k] = t;
            for (int q = 0; q < 4; q++) { const float v = Vt[i][q]; Vt[i][q] = Vt[k][q]; Vt[k][q] = v; }
        }
    }
    for (int q = 0; q < 4; q++) x[q] = Vt[3][q];
}

// KeyFrame::UnprojectStereo(idx) with z > 0 (the entry points refuse a stereo key without depth: the reference would go on with an empty matrix)
SIND_HD inline void mp_unproject_stereo(const TriCam& c, const float* Twc, const float* xy, float z, float* X) {
    const float x = (xy[0] - c.cx) * z * c.invfx, y = (xy[1] - c.cy) * z * c.invfy;
    for (int r = 0; r < 3; r++) {
        const float t = Twc[4 * r] * x + Twc[4 * r + 1] * y + Twc[4 * r + 2] * z;
        X[r] = (float)((double)t * 1.0 + (double)Twc[4 * r + 3] * 1.0);
    }
}

// one pass of the loop body of :286-450 up to `new MapPoint`
SIND_HD inline void tri_point(const TriCam& c, const TriPair& P, const TriMatch& q, TriOut& o) {
    o.x3D[0] = o.x3D[1] = o.x3D[2] = 0.f; o.how = -1; o.status = TRI_LOW_PARALLAX;
    const bool st1 = q.ur1 >= 0, st2 = q.ur2 >= 0;
    const float xn1[3] = {(q.un1[0] - c.cx) * c.invfx, (q.un1[1] - c.cy) * c.invfy, 1.0f};
    const float xn2[3] = {(q.un2[0] - c.cx) * c.invfx, (q.un2[1] - c.cy) * c.invfy, 1.0f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) {
        ray1[r] = P.Tcw1[r] * xn1[0] + P.Tcw1[4 + r] * xn1[1] + P.Tcw1[8 + r] * xn1[2];
        ray2[r] = P.Tcw2[r] * xn2[0] + P.Tcw2[4 + r] * xn2[1] + P.Tcw2[8 + r] * xn2[2];
    }
    const float cosRays = (float)(mp_dot3(ray1, ray2) / (mp_norm3(ray1) * mp_norm3(ray2)));
    float cs1 = cosRays + 1, cs2 = cs1;
    if (st1) cs1 = q.cos1; else if (st2) cs2 = q.cos2;
    const float cs = cs2 < cs1 ? cs2 : cs1;
    float X[3];
    if (cosRays < cs && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float At[4][4], x[4];
        for (int k = 0; k < 4; k++) {
            At[k][0] = P.Tcw1[8 + k] * xn1[0] - P.Tcw1[k];
            At[k][1] = P.Tcw1[8 + k] * xn1[1] - P.Tcw1[4 + k];
            At[k][2] = P.Tcw2[8 + k] * xn2[0] - P.Tcw2[k];
            At[k][3] = P.Tcw2[8 + k] * xn2[1] - P.Tcw2[4 + k];
        }
        mp_svd4_last_row(At, x);
        o.how = 0;
        if (x[3] == 0) { o.status = TRI_W0; return; }
        const float inv = (float)(1.0 / (double)x[3]);
        for (int k = 0; k < 3; k++) X[k] = x[k] * inv;
    } else if (st1 && cs1 < cs2) { o.how = 1; mp_unproject_stereo(c, P.Twc1, q.xy1, q.depth1, X); }
    else if (st2 && cs2 < cs1) { o.how = 2; mp_unproject_stereo(c, P.Twc2, q.xy2, q.depth2, X); }
    else return;                                                      // no stereo and very low parallax
    for (int k = 0; k < 3; k++) o.x3D[k] = X[k];
    const float z1 = (float)(mp_dot3(P.Tcw1 + 8, X) + (double)P.Tcw1[11]);
    if (z1 <= 0) { o.status = TRI_Z1; return; }
    const float z2 = (float)(mp_dot3(P.Tcw2 + 8, X) + (double)P.Tcw2[11]);
    if (z2 <= 0) { o.status = TRI_Z2; return; }
    {
        const float s2 = c.sigma2[q.oct1];
        const float x1 = (float)(mp_dot3(P.Tcw1, X) + (double)P.Tcw1[3]), y1 = (float)(mp_dot3(P.Tcw1 + 4, X) + (double)P.Tcw1[7]);
        const float invz = (float)(1.0 / (double)z1);
        const float u = c.fx * x1 * invz + c.cx, v = c.fy * y1 * invz + c.cy, ex = u - q.un1[0], ey = v - q.un1[1];
        if (!st1) { if ((double)(ex * ex + ey * ey) > 5.991 * (double)s2) { o.status = TRI_REPROJ1; return; } }
        else { const float ur = u - c.bf * invz, er = ur - q.ur1; if ((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)s2) { o.status = TRI_REPROJ1; return; } }
    }
    {
        const float s2 = c.sigma2[q.oct2];
        const float x2 = (float)(mp_dot3(P.Tcw2, X) + (double)P.Tcw2[3]), y2 = (float)(mp_dot3(P.Tcw2 + 4, X) + (double)P.Tcw2[7]);
        const float invz = (float)(1.0 / (double)z2);
        const float u = c.fx * x2 * invz + c.cx, v = c.fy * y2 * invz + c.cy, ex = u - q.un2[0], ey = v - q.un2[1];
        if (!st2) { if ((double)(ex * ex + ey * ey) > 5.991 * (double)s2) { o.status = TRI_REPROJ2; return; } }
        else { const float ur = u - c.bf * invz, er = ur - q.ur2; if ((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)s2) { o.status = TRI_REPROJ2; return; } }
    }
    const float n1[3] = {X[0] - P.Twc1[3], X[1] - P.Twc1[7], X[2] - P.Twc1[11]}, n2[3] = {X[0] - P.Twc2[3], X[1] - P.Twc2[7], X[2] - P.Twc2[11]};
    const float dist1 = (float)mp_norm3(n1), dist2 = (float)mp_norm3(n2);
    if (dist1 == 0 || dist2 == 0) { o.status = TRI_DIST0; return; }
    const float ratioDist = dist2 / dist1, ratioOctave = c.scale[q.oct1] / c.scale[q.oct2];
    if (ratioDist * c.ratioFactor < ratioOctave || ratioDist > ratioOctave * c.ratioFactor) { o.status = TRI_SCALE; return; }
    o.status = TRI_NEW;
}

// The points of every item of a sind_match_update_points call, one after the other; pointers of the host or of the device.  Every index was checked before the kernels see it.
struct MpCam { float scale[16]; int nlevels; };
struct MpArrays {
    const int* obsFirst; const int* obsCount;                        // [nPts]: the point's observations are obsFirst .. obsFirst + obsCount - 1 of the call's observations
    const uint8_t* todo;                                             // [nPts]: bit 0 do_descriptor, bit 1 do_normal of the point's item
    const float* x3Dw; const int* refObs;                            // [nPts][3], [nPts]: the position of mpRefKF in the point's own list
    const int* obsKf; const uint8_t* obsBad; const int* obsOctave; const uint32_t* obsDesc;      // [nObs] (index into Ow, of the whole call), .., .., [nObs][8]
    const float* Ow;                                                 // [nKf][3] of the whole call
    uint32_t* descOut; int* bestObs; float* normal; float* maxDist; float* minDist; uint8_t* updated;      // [nPts][8], [nPts], [nPts][3], [nPts] x 3
};

// MapPoint::UpdateNormalAndDepth of point j
SIND_HD inline void mp_normal_depth(const MpCam& c, const MpArrays& a, int j) {
    const int first = a.obsFirst[j], n = a.obsCount[j];
    if (n == 0) { a.updated[j] = 0; return; }
    const float* P = a.x3Dw + 3 * (size_t)j;
    float N[3] = {0.f, 0.f, 0.f};
    for (int e = first; e < first + n; e++) {
        const float* O = a.Ow + 3 * (size_t)a.obsKf[e];
        const float d[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
        const float inv = (float)(1.0 / mp_norm3(d));
        for (int k = 0; k < 3; k++) N[k] = d[k] * inv + N[k];
    }
    const int r = first + a.refObs[j];
    const float* O = a.Ow + 3 * (size_t)a.obsKf[r];
    const float pc[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
    const float dist = (float)mp_norm3(pc);
    const float maxD = dist * c.scale[a.obsOctave[r]];
    a.maxDist[j] = maxD; a.minDist[j] = maxD / c.scale[c.nlevels - 1];
    const float invn = (float)(1.0 / (double)n);
    for (int k = 0; k < 3; k++) a.normal[3 * (size_t)j + k] = N[k] * invn;
    a.updated[j] = 1;
}

// map_points.cpp: what the entry points of both libraries share
struct MpFill { int* obsFirst; int* obsCount; uint8_t* todo; float* x3Dw; int* refObs; int* obsKf; uint8_t* obsBad; int* obsOctave; uint32_t* obsDesc; float* Ow; };
extern const char* const tri_check_text[];
extern const char* const mpu_check_text[];
void tri_cam(const float* K5, const float* scale, int nlevels, TriCam& c);
int tri_check(const ::sind_tri_pair& q, int nlevels);                                   // -> 0, or the index into tri_check_text
void tri_pair(const ::sind_tri_pair& q, TriPair& P);
void tri_collect(const ::sind_tri_pair& q, int b, float mb, std::vector<TriMatch>& out);
void tri_store(const ::sind_tri_pair& q, int b, const TriMatch* m, const TriOut* o, size_t count);
int mpu_check(const ::sind_mappoints_item& q, int nlevels, bool contents);              // -> 0, or the index into mpu_check_text
bool mpu_over_limit(const ::sind_mappoints_item& q);
void mpu_totals(const ::sind_mappoints_item* items, int B, size_t& nKf, size_t& nPts, size_t& nObs);
void mpu_fill(const ::sind_mappoints_item* items, int B, const MpFill& h);
void mpu_store(const ::sind_mappoints_item* items, int B, const MpArrays& a);

}  // namespace sind
