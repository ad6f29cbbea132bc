// Host twins of sind_match_triangulate and sind_match_update_points (reference src/LocalMapping.cc:284-431, src/MapPoint.cc:242-307, :330-371): map_points.hpp run
// match after match and point after point, MapPoint::ComputeDistinctiveDescriptors transcribed literally, and what the entry points of both libraries share: the
// argument checks, the list of matches with the stereo parallax cosines (evaluated HERE with the C library, never on the device), the flattening of the items of an
// update and the copies of the results.  Compiled into libsind_hip.so (capi_match_map.cpp calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#include "map_points.hpp"
#include "sind_hip.h"

namespace sind {

const char* const tri_check_text[] = {"", "negative count", "null array", "a match12 entry outside [-1, n2)", "an octave outside [0, nlevels)", "a pose is not finite",
                                      "a matched stereo keypoint without depth"};
const char* const mpu_check_text[] = {"", "negative count", "null array", "obs_start does not start at 0 or decreases", "an obs_kf is out of range", "an obs_octave is out of range",
                                      "a ref_obs is out of range", "ref_obs = -1 on a point with observations while do_normal is set", "a position or camera centre is not finite"};

void tri_cam(const float* K5, const float* scale, int nlevels, TriCam& c) {
    c.fx = K5[0]; c.fy = K5[1]; c.cx = K5[2]; c.cy = K5[3]; c.bf = K5[4];
    c.invfx = 1.0f / c.fx; c.invfy = 1.0f / c.fy;                   // Frame.cc:152-153
    for (int l = 0; l < 16; l++) { c.scale[l] = l < nlevels ? scale[l] : 0.f; c.sigma2[l] = c.scale[l] * c.scale[l]; }
    c.ratioFactor = 1.5f * c.scale[1];
}

static bool side_null(const ::sind_tri_side& s) { return s.n && (!s.xy || !s.un_xy || !s.octave || !s.u_right || !s.depth); }

int tri_check(const ::sind_tri_pair& q, int nlevels) {
    if (q.kf1.n < 0 || q.kf2.n < 0) return 1;
    if (!q.Tcw1 || !q.Twc1 || !q.Tcw2 || !q.Twc2 || !q.nnew || side_null(q.kf1) || side_null(q.kf2) || (q.kf1.n && (!q.match12 || !q.x3D || !q.how || !q.status))) return 2;
    for (int i = 0; i < q.kf1.n; i++) if (q.match12[i] < -1 || q.match12[i] >= q.kf2.n) return 3;
    for (const ::sind_tri_side* s : {&q.kf1, &q.kf2}) for (int i = 0; i < s->n; i++) if (s->octave[i] < 0 || s->octave[i] >= nlevels) return 4;
    for (const float* T : {q.Tcw1, q.Twc1, q.Tcw2, q.Twc2}) for (int k = 0; k < 16; k++) if (!std::isfinite(T[k])) return 5;
    for (int i = 0; i < q.kf1.n; i++) {
        const int j = q.match12[i];
        if (j >= 0 && ((q.kf1.u_right[i] >= 0 && !(q.kf1.depth[i] > 0)) || (q.kf2.u_right[j] >= 0 && !(q.kf2.depth[j] > 0)))) return 6;
    }
    return 0;
}

void tri_pair(const ::sind_tri_pair& q, TriPair& P) {
    std::memcpy(P.Tcw1, q.Tcw1, sizeof(P.Tcw1)); std::memcpy(P.Twc1, q.Twc1, sizeof(P.Twc1)); std::memcpy(P.Tcw2, q.Tcw2, sizeof(P.Tcw2)); std::memcpy(P.Twc2, q.Twc2, sizeof(P.Twc2));
}

// cos(2*atan2(mb/2, depth)) of :312 and :314: the float overloads (map_points.hpp), the C library's
static float stereo_cos(float mb, float depth) { return std::cos(2 * std::atan2(mb / 2, depth)); }

// vMatchedIndices of pair b, in ascending idx1, appended to out
void tri_collect(const ::sind_tri_pair& q, int b, float mb, std::vector<TriMatch>& out) {
    for (int i = 0; i < q.kf1.n; i++) {
        const int j = q.match12[i];
        if (j < 0) continue;
        TriMatch t{};
        t.un1[0] = q.kf1.un_xy[2 * i]; t.un1[1] = q.kf1.un_xy[2 * i + 1]; t.xy1[0] = q.kf1.xy[2 * i]; t.xy1[1] = q.kf1.xy[2 * i + 1]; t.ur1 = q.kf1.u_right[i]; t.depth1 = q.kf1.depth[i]; t.oct1 = q.kf1.octave[i];
        t.un2[0] = q.kf2.un_xy[2 * j]; t.un2[1] = q.kf2.un_xy[2 * j + 1]; t.xy2[0] = q.kf2.xy[2 * j]; t.xy2[1] = q.kf2.xy[2 * j + 1]; t.ur2 = q.kf2.u_right[j]; t.depth2 = q.kf2.depth[j]; t.oct2 = q.kf2.octave[j];
        if (t.ur1 >= 0) t.cos1 = stereo_cos(mb, t.depth1); else if (t.ur2 >= 0) t.cos2 = stereo_cos(mb, t.depth2);
        t.pair = b; t.idx1 = i;
        out.push_back(t);
    }
}

// the outputs of pair b from the count matches of the call; "no match" elsewhere
void tri_store(const ::sind_tri_pair& q, int b, const TriMatch* m, const TriOut* o, size_t count) {
    for (int i = 0; i < q.kf1.n; i++) { q.x3D[3 * i] = q.x3D[3 * i + 1] = q.x3D[3 * i + 2] = 0.f; q.how[i] = -1; q.status[i] = -1; }
    int nnew = 0;
    for (size_t k = 0; k < count; k++) if (m[k].pair == b) {
        const int i = m[k].idx1;
        std::memcpy(q.x3D + 3 * i, o[k].x3D, sizeof(o[k].x3D)); q.how[i] = o[k].how; q.status[i] = o[k].status; nnew += o[k].status == TRI_NEW;
    }
    *q.nnew = nnew;
}

static int n_obs(const ::sind_mappoints_item& q) { return q.n_mp ? q.obs_start[q.n_mp] : 0; }

// contents = false: the counts, the NULL arrays and obs_start alone, which is what the limits read
int mpu_check(const ::sind_mappoints_item& q, int nlevels, bool contents) {
    if (q.n_kf < 0 || q.n_mp < 0) return 1;
    if ((q.n_kf && !q.Ow) || (q.n_mp && (!q.x3Dw || !q.obs_start || !q.ref_obs))) return 2;
    if (q.n_mp && q.do_descriptor && (!q.desc_out || !q.best_obs)) return 2;
    if (q.n_mp && q.do_normal && (!q.normal_out || !q.max_dist || !q.min_dist || !q.updated)) return 2;
    if (q.n_mp) { if (q.obs_start[0] != 0) return 3; for (int j = 0; j < q.n_mp; j++) if (q.obs_start[j + 1] < q.obs_start[j]) return 3; }
    const int nObs = n_obs(q);
    if (nObs && (!q.obs_kf || !q.obs_bad || !q.obs_octave || !q.obs_desc)) return 2;
    if (!contents) return 0;
    for (int e = 0; e < nObs; e++) { if (q.obs_kf[e] < 0 || q.obs_kf[e] >= q.n_kf) return 4; if (q.obs_octave[e] < 0 || q.obs_octave[e] >= nlevels) return 5; }
    for (int j = 0; j < q.n_mp; j++) {
        const int c = q.obs_start[j + 1] - q.obs_start[j];
        if (q.ref_obs[j] < -1 || q.ref_obs[j] >= c) return 6;
        if (q.do_normal && c && q.ref_obs[j] < 0) return 7;
    }
    for (size_t k = 0; k < (size_t)3 * q.n_kf; k++) if (!std::isfinite(q.Ow[k])) return 8;
    for (size_t k = 0; k < (size_t)3 * q.n_mp; k++) if (!std::isfinite(q.x3Dw[k])) return 8;
    return 0;
}

bool mpu_over_limit(const ::sind_mappoints_item& q) {               // after mpu_check(.., false)
    return q.n_kf > MPU_MAX_KF || q.n_mp > MPU_MAX_MP || n_obs(q) > MPU_MAX_OBS;
}

void mpu_totals(const ::sind_mappoints_item* items, int B, size_t& nKf, size_t& nPts, size_t& nObs) {
    nKf = nPts = nObs = 0;
    for (int b = 0; b < B; b++) { nKf += (size_t)items[b].n_kf; nPts += (size_t)items[b].n_mp; nObs += (size_t)n_obs(items[b]); }
}

// the items of a call one after the other in the arrays of h (sized by mpu_totals; the inputs are written)
void mpu_fill(const ::sind_mappoints_item* items, int B, const MpFill& h) {
    size_t kf0 = 0, pt0 = 0, ob0 = 0;
    for (int b = 0; b < B; b++) {
        const ::sind_mappoints_item& q = items[b]; const int nObs = n_obs(q);
        if (q.n_kf) std::memcpy(h.Ow + 3 * kf0, q.Ow, sizeof(float) * 3 * (size_t)q.n_kf);
        if (q.n_mp) std::memcpy(h.x3Dw + 3 * pt0, q.x3Dw, sizeof(float) * 3 * (size_t)q.n_mp);
        for (int j = 0; j < q.n_mp; j++) {
            h.obsFirst[pt0 + j] = (int)ob0 + q.obs_start[j]; h.obsCount[pt0 + j] = q.obs_start[j + 1] - q.obs_start[j]; h.refObs[pt0 + j] = q.ref_obs[j];
            h.todo[pt0 + j] = (uint8_t)((q.do_descriptor ? 1 : 0) | (q.do_normal ? 2 : 0));
        }
        for (int e = 0; e < nObs; e++) { h.obsKf[ob0 + e] = (int)kf0 + q.obs_kf[e]; h.obsBad[ob0 + e] = q.obs_bad[e] ? 1 : 0; h.obsOctave[ob0 + e] = q.obs_octave[e]; }
        if (nObs) std::memcpy(h.obsDesc + 8 * ob0, q.obs_desc, (size_t)32 * nObs);
        kf0 += (size_t)q.n_kf; pt0 += (size_t)q.n_mp; ob0 += (size_t)nObs;
    }
}

// the outputs of every item from the call's arrays (host pointers): only what the reference writes
void mpu_store(const ::sind_mappoints_item* items, int B, const MpArrays& a) {
    size_t pt0 = 0;
    for (int b = 0; b < B; b++) {
        const ::sind_mappoints_item& q = items[b];
        for (int j = 0; j < q.n_mp; j++) {
            const size_t g = pt0 + j;
            if (q.do_descriptor) { q.best_obs[j] = a.bestObs[g]; if (a.bestObs[g] >= 0) std::memcpy(q.desc_out + 32 * (size_t)j, a.descOut + 8 * g, 32); }
            if (q.do_normal) {
                q.updated[j] = a.updated[g];
                if (a.updated[g]) { std::memcpy(q.normal_out + 3 * (size_t)j, a.normal + 3 * g, 12); q.max_dist[j] = a.maxDist[g]; q.min_dist[j] = a.minDist[g]; }
            }
        }
        pt0 += (size_t)q.n_mp;
    }
}

static int descriptor_distance(const uint32_t* a, const uint32_t* b) { int d = 0; for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]); return d; }

// MapPoint::ComputeDistinctiveDescriptors of point j, as written: vDescriptors, Distances[N][N], the sorted row, vDists[0.5 * (N - 1)]
static void descriptor_literal(const MpArrays& a, int j) {
    const int first = a.obsFirst[j], n = a.obsCount[j];
    std::vector<int> v;                                              // positions in the point's list of the observers that are not bad
    for (int e = 0; e < n; e++) if (!a.obsBad[first + e]) v.push_back(e);
    if (v.empty()) { a.bestObs[j] = -1; return; }
    const size_t N = v.size();
    std::vector<float> D(N * N);
    for (size_t i = 0; i < N; i++) {
        D[i * N + i] = 0;
        for (size_t k = i + 1; k < N; k++) { const int d = descriptor_distance(a.obsDesc + 8 * (size_t)(first + v[i]), a.obsDesc + 8 * (size_t)(first + v[k])); D[i * N + k] = (float)d; D[k * N + i] = (float)d; }
    }
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(D.begin() + i * N, D.begin() + (i + 1) * N);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    a.bestObs[j] = v[BestIdx];
    std::memcpy(a.descOut + 8 * (size_t)j, a.obsDesc + 8 * (size_t)(first + v[BestIdx]), 32);
}

}  // namespace sind

extern "C" {

// the same pairs as sind_match_triangulate, match after match on the CPU.  -> 0, or SIND_E_ARG with nothing written
int sindh_triangulate(const sind_tri_pair* pairs, int B, const float* K5, const float* scale_factors, int nlevels) {
    if (B < 0 || (B && !pairs) || !K5 || !scale_factors || nlevels < 2 || nlevels > 16) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::tri_check(pairs[b], nlevels)) return SIND_E_ARG;
    sind::TriCam c; sind::tri_cam(K5, scale_factors, nlevels, c);
    const float mb = K5[4] / K5[0];                                  // Frame.cc:167
    std::vector<sind::TriMatch> ms;
    for (int b = 0; b < B; b++) sind::tri_collect(pairs[b], b, mb, ms);
    std::vector<sind::TriOut> out(ms.size());
    for (size_t k = 0; k < ms.size(); k++) { sind::TriPair P; sind::tri_pair(pairs[ms[k].pair], P); sind::tri_point(c, P, ms[k], out[k]); }
    for (int b = 0; b < B; b++) sind::tri_store(pairs[b], b, ms.data(), out.data(), ms.size());
    return SIND_OK;
}

// the same items as sind_match_update_points, point after point on the CPU.  -> 0, or SIND_E_ARG with nothing written
int sindh_update_points(const sind_mappoints_item* items, int B, const float* scale_factors, int nlevels) {
    if (B < 0 || (B && !items) || !scale_factors || nlevels < 1 || nlevels > 16) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::mpu_check(items[b], nlevels, true)) return SIND_E_ARG;
    size_t nKf, nPts, nObs; sind::mpu_totals(items, B, nKf, nPts, nObs);
    std::vector<int> obsFirst(nPts + 1), obsCount(nPts + 1), refObs(nPts + 1), obsKf(nObs + 1), obsOctave(nObs + 1), bestObs(nPts + 1);
    std::vector<uint8_t> todo(nPts + 1), obsBad(nObs + 1), updated(nPts + 1);
    std::vector<float> x3Dw(3 * nPts + 1), Ow(3 * nKf + 1), normal(3 * nPts + 1), maxDist(nPts + 1), minDist(nPts + 1);
    std::vector<uint32_t> obsDesc(8 * nObs + 1), descOut(8 * nPts + 1);
    sind::mpu_fill(items, B, sind::MpFill{obsFirst.data(), obsCount.data(), todo.data(), x3Dw.data(), refObs.data(), obsKf.data(), obsBad.data(), obsOctave.data(), obsDesc.data(), Ow.data()});
    const sind::MpArrays a{obsFirst.data(), obsCount.data(), todo.data(), x3Dw.data(), refObs.data(), obsKf.data(), obsBad.data(), obsOctave.data(), obsDesc.data(), Ow.data(),
                           descOut.data(), bestObs.data(), normal.data(), maxDist.data(), minDist.data(), updated.data()};
    sind::MpCam c{}; for (int l = 0; l < nlevels; l++) c.scale[l] = scale_factors[l]; c.nlevels = nlevels;
    for (size_t j = 0; j < nPts; j++) {
        if (todo[j] & 1) sind::descriptor_literal(a, (int)j);
        if (todo[j] & 2) sind::mp_normal_depth(c, a, (int)j);
    }
    sind::mpu_store(items, B, a);
    return SIND_OK;
}

}  // extern "C"
