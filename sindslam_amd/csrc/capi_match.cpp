// C ABI: projection matcher (include/sind_hip.h, "sind_match_*").
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "match.hpp"

struct sind_match {
    int device = 0, maxB = 0; sind::MatchParams prm{}; float mb = 0; hipStream_t stream = nullptr;
    DevBuf<sind::MatchPose> pose; DevBuf<int> nLast, nCur, lastOct, curOct, gstart, gidx, choice, minOwner, matchOfCur, nmatches, rounds;
    DevBuf<float> x3Dw, lastAng, curXY, curAng, curUR; DevBuf<uint8_t> lastFlags, curTaken; DevBuf<uint32_t> lastDesc, curDesc;
    // host staging (one H2D per array and call)
    std::vector<sind::MatchPose> h_pose; std::vector<int> h_nLast, h_nCur, h_lastOct, h_curOct, h_gstart, h_gidx, h_match, h_nm, h_rounds;
    std::vector<float> h_x3Dw, h_lastAng, h_curXY, h_curAng, h_curUR; std::vector<uint8_t> h_lastFlags, h_curTaken, h_lastDesc, h_curDesc;
    int last_rounds = 0;
    DevBuf<float4> curPack;                                        // keypoint records of match_local.hip, on first use
    // map-point side of sind_match_local_map (capacity from sind_match_reserve_map_points) and of sind_match_by_projection_kf (cap_last, on first use)
    struct PointSide {
        int cap = 0;
        DevBuf<sind::LocalPose> pose; DevBuf<int> nPts, level, choice, nToMatch; DevBuf<float> x3Dw, normal, maxDist, minDist, angle, projXYR, viewCos;
        DevBuf<uint8_t> flags, inView; DevBuf<uint32_t> desc;
        std::vector<sind::LocalPose> h_pose; std::vector<int> h_nPts, h_level, h_nToMatch; std::vector<float> h_x3Dw, h_normal, h_maxDist, h_minDist, h_angle, h_projXYR, h_viewCos;
        std::vector<uint8_t> h_flags, h_inView, h_desc;
        int reserve(size_t B, int c) {
            const size_t n = B * (size_t)c; int r = SIND_OK;
            if ((r = pose.alloc(B)) || (r = nPts.alloc(B)) || (r = nToMatch.alloc(B)) || (r = level.alloc(n)) || (r = choice.alloc(n)) || (r = x3Dw.alloc(n * 3)) || (r = normal.alloc(n * 3)) ||
                (r = maxDist.alloc(n)) || (r = minDist.alloc(n)) || (r = angle.alloc(n)) || (r = projXYR.alloc(n * 3)) || (r = viewCos.alloc(n)) || (r = flags.alloc(n)) || (r = inView.alloc(n)) ||
                (r = desc.alloc(n * 8))) return r;
            h_pose.resize(B); h_nPts.resize(B); h_nToMatch.resize(B); h_level.resize(n); h_x3Dw.resize(n * 3); h_normal.resize(n * 3); h_maxDist.resize(n); h_minDist.resize(n); h_angle.resize(n);
            h_projXYR.resize(n * 3); h_viewCos.resize(n); h_flags.resize(n); h_inView.resize(n); h_desc.resize(n * 32);
            cap = c; return SIND_OK;
        }
    } local, reloc;
    // node ids, sort scratch and the extra key-frame arrays of sind_match_by_bow / sind_match_for_triangulation (match_bow.hip), on first use
    struct BowSide {
        bool ready = false;
        DevBuf<int> nodeA, nodeB, segStart, nSeg, nValid; DevBuf<int2> sortedA, sortedB; DevBuf<float> lastXY, lastUR; DevBuf<sind::TriPose> pose;
        std::vector<int> h_nodeA, h_nodeB, h_match12; std::vector<float> h_lastXY, h_lastUR; std::vector<sind::TriPose> h_pose;
        int reserve(size_t B, size_t cl, size_t cc) {
            if (ready) return SIND_OK;
            int r = SIND_OK;
            if ((r = nodeA.alloc(B * cl)) || (r = nodeB.alloc(B * cc)) || (r = segStart.alloc(B * cl)) || (r = nSeg.alloc(B)) || (r = nValid.alloc(2 * B)) || (r = sortedA.alloc(B * cl)) ||
                (r = sortedB.alloc(B * cc)) || (r = lastXY.alloc(B * cl * 2)) || (r = lastUR.alloc(B * cl)) || (r = pose.alloc(B))) return r;
            h_nodeA.resize(B * cl); h_nodeB.resize(B * cc); h_match12.resize(B * cl); h_lastXY.resize(B * cl * 2); h_lastUR.resize(B * cl); h_pose.resize(B);
            ready = true; return SIND_OK;
        }
    } bow;
};

// CurrentFrame / LastFrame pose algebra of ORBmatcher.cc:1338-1349 (cv::gemm semantics: A*b+c without transposition = FP32 row
// product then FP64 alpha/beta; -A^T*b = FP64 accumulation)
static void forward_backward(const float* Tc, const float* Tl, float mb, bool mono, int& fwd, int& bwd) {
    float twc[3], tlc[3];
    for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)Tc[4 * k + r] * (double)Tc[4 * k + 3]; twc[r] = (float)(s * -1.0); }
    for (int r = 0; r < 3; r++) { const float t = Tl[4 * r] * twc[0] + Tl[4 * r + 1] * twc[1] + Tl[4 * r + 2] * twc[2]; tlc[r] = (float)((double)t * 1.0 + (double)Tl[4 * r + 3] * 1.0); }
    fwd = tlc[2] > mb && !mono; bwd = -tlc[2] > mb && !mono;
}

template <class T> static int up(DevBuf<T>& d, const std::vector<T>& h, size_t n, hipStream_t s) { HIP_TRY(hipMemcpyAsync(d.p, h.data(), n * sizeof(T), hipMemcpyHostToDevice, s)); return SIND_OK; }

extern "C" {

int sind_match_create(const sind_match_config* c, sind_match** out) {
    if (!c || !out || c->cap_last < 1 || c->cap_cur < 1 || c->max_batch < 1 || c->nlevels < 1 || c->nlevels > 16 || !(c->fx > 0)) { sind_set_error("sind_match_create: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    sind_match* m = new sind_match(); m->device = c->device; m->maxB = c->max_batch;
    sind::MatchParams& p = m->prm; p.fx = c->fx; p.fy = c->fy; p.cx = c->cx; p.cy = c->cy; p.bf = c->bf; std::memcpy(p.bounds, c->bounds, sizeof(p.bounds));
    for (int i = 0; i < 16; i++) p.scale[i] = i < c->nlevels ? c->scale_factors[i] : 0.f;
    p.nlevels = c->nlevels; p.capLast = c->cap_last; p.capCur = c->cap_cur; m->mb = c->bf / c->fx;                 // Frame.cc:167 mb = mbf / fx
    const size_t B = c->max_batch, nl = B * c->cap_last, nc = B * c->cap_cur;
    int r = SIND_OK;
    if ((r = m->pose.alloc(B)) || (r = m->nLast.alloc(B)) || (r = m->nCur.alloc(B)) || (r = m->lastOct.alloc(nl)) || (r = m->curOct.alloc(nc)) || (r = m->gstart.alloc(B * 3073)) ||
        (r = m->gidx.alloc(nc)) || (r = m->choice.alloc(nl)) || (r = m->minOwner.alloc(nc)) || (r = m->matchOfCur.alloc(nc)) || (r = m->nmatches.alloc(B)) || (r = m->rounds.alloc(B)) ||
        (r = m->x3Dw.alloc(nl * 3)) || (r = m->lastAng.alloc(nl)) || (r = m->curXY.alloc(nc * 2)) || (r = m->curAng.alloc(nc)) || (r = m->curUR.alloc(nc)) || (r = m->lastFlags.alloc(nl)) ||
        (r = m->curTaken.alloc(nc)) || (r = m->lastDesc.alloc(nl * 8)) || (r = m->curDesc.alloc(nc * 8))) { delete m; return r; }
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; sind_set_error("sind_match_create: stream creation failed"); return SIND_E_HIP; }
    m->h_pose.resize(B); m->h_nLast.resize(B); m->h_nCur.resize(B); m->h_lastOct.resize(nl); m->h_curOct.resize(nc); m->h_gstart.resize(B * 3073); m->h_gidx.resize(nc); m->h_match.resize(nc);
    m->h_nm.resize(B); m->h_rounds.resize(B); m->h_x3Dw.resize(nl * 3); m->h_lastAng.resize(nl); m->h_curXY.resize(nc * 2); m->h_curAng.resize(nc); m->h_curUR.resize(nc);
    m->h_lastFlags.resize(nl); m->h_curTaken.resize(nc); m->h_lastDesc.resize(nl * 32); m->h_curDesc.resize(nc * 32);
    *out = m; return SIND_OK;
}
int sind_match_destroy(sind_match* m) {
    if (!m) return SIND_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    hipStream_t s = m->stream; delete m; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}

int sind_match_by_projection(sind_match* m, const sind_match_pair* pairs, int B, float th, int mono, int check_orientation) {
    if (!m || !pairs || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_by_projection: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    sind::MatchParams p = m->prm; p.th = th; p.checkOrientation = check_orientation ? 1 : 0;
    const int cl = p.capLast, cc = p.capCur;
    for (int b = 0; b < B; b++) {
        const sind_match_pair& q = pairs[b];
        if (q.n_last < 0 || q.n_last > cl || q.n_cur < 0 || q.n_cur > cc) { sind_set_error("sind_match_by_projection: pair %d has %d / %d points, capacity %d / %d", b, q.n_last, q.n_cur, cl, cc); return SIND_E_CAPACITY; }
        if (!q.Tcw_cur || !q.Tcw_last || !q.match_of_cur || !q.nmatches || (q.n_last && (!q.x3Dw || !q.last_valid || !q.last_has_obs || !q.last_octave || !q.last_angle || !q.last_desc)) ||
            (q.n_cur && (!q.cur_un_xy || !q.cur_octave || !q.cur_angle || !q.cur_u_right || !q.cur_desc || !q.grid_idx)) || !q.grid_start) { sind_set_error("sind_match_by_projection: null array in pair %d", b); return SIND_E_ARG; }
        sind::MatchPose& ps = m->h_pose[b]; std::memcpy(ps.Tcw, q.Tcw_cur, sizeof(ps.Tcw));
        forward_backward(q.Tcw_cur, q.Tcw_last, m->mb, mono != 0, ps.forward, ps.backward);
        m->h_nLast[b] = q.n_last; m->h_nCur[b] = q.n_cur;
        for (int i = 0; i < q.n_last; i++) {
            if (q.last_octave[i] < 0 || q.last_octave[i] >= p.nlevels) { sind_set_error("sind_match_by_projection: octave %d outside [0,%d)", q.last_octave[i], p.nlevels); return SIND_E_ARG; }
            m->h_lastFlags[(size_t)b * cl + i] = (uint8_t)((q.last_valid[i] ? 1 : 0) | (q.last_has_obs[i] ? 2 : 0));
        }
        std::memcpy(&m->h_x3Dw[(size_t)b * cl * 3], q.x3Dw, (size_t)q.n_last * 12); std::memcpy(&m->h_lastOct[(size_t)b * cl], q.last_octave, (size_t)q.n_last * 4);
        std::memcpy(&m->h_lastAng[(size_t)b * cl], q.last_angle, (size_t)q.n_last * 4); std::memcpy(&m->h_lastDesc[(size_t)b * cl * 32], q.last_desc, (size_t)q.n_last * 32);
        std::memcpy(&m->h_curXY[(size_t)b * cc * 2], q.cur_un_xy, (size_t)q.n_cur * 8); std::memcpy(&m->h_curOct[(size_t)b * cc], q.cur_octave, (size_t)q.n_cur * 4);
        std::memcpy(&m->h_curAng[(size_t)b * cc], q.cur_angle, (size_t)q.n_cur * 4); std::memcpy(&m->h_curUR[(size_t)b * cc], q.cur_u_right, (size_t)q.n_cur * 4);
        std::memcpy(&m->h_curDesc[(size_t)b * cc * 32], q.cur_desc, (size_t)q.n_cur * 32);
        if (q.grid_start[0] != 0 || q.grid_start[3072] < 0 || q.grid_start[3072] > q.n_cur) { sind_set_error("sind_match_by_projection: malformed grid of pair %d", b); return SIND_E_ARG; }
        for (int c = 0; c < 3072; c++) if (q.grid_start[c + 1] < q.grid_start[c]) { sind_set_error("sind_match_by_projection: malformed grid of pair %d", b); return SIND_E_ARG; }
        for (int j = 0; j < q.grid_start[3072]; j++) if (q.grid_idx[j] < 0 || q.grid_idx[j] >= q.n_cur) { sind_set_error("sind_match_by_projection: grid index outside the keypoints (pair %d)", b); return SIND_E_ARG; }
        std::memcpy(&m->h_gstart[(size_t)b * 3073], q.grid_start, 3073 * 4); std::memcpy(&m->h_gidx[(size_t)b * cc], q.grid_idx, (size_t)q.grid_start[3072] * 4);
        if (q.cur_taken) std::memcpy(&m->h_curTaken[(size_t)b * cc], q.cur_taken, q.n_cur); else std::memset(&m->h_curTaken[(size_t)b * cc], 0, q.n_cur);
    }
    hipStream_t s = m->stream; const size_t nl = (size_t)B * cl, nc = (size_t)B * cc;
    SIND_TRY(up(m->pose, m->h_pose, B, s)); SIND_TRY(up(m->nLast, m->h_nLast, B, s)); SIND_TRY(up(m->nCur, m->h_nCur, B, s)); SIND_TRY(up(m->x3Dw, m->h_x3Dw, nl * 3, s));
    SIND_TRY(up(m->lastFlags, m->h_lastFlags, nl, s)); SIND_TRY(up(m->lastOct, m->h_lastOct, nl, s)); SIND_TRY(up(m->lastAng, m->h_lastAng, nl, s));
    HIP_TRY(hipMemcpyAsync(m->lastDesc.p, m->h_lastDesc.data(), nl * 32, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(m->curDesc.p, m->h_curDesc.data(), nc * 32, hipMemcpyHostToDevice, s));
    SIND_TRY(up(m->curXY, m->h_curXY, nc * 2, s)); SIND_TRY(up(m->curOct, m->h_curOct, nc, s)); SIND_TRY(up(m->curAng, m->h_curAng, nc, s)); SIND_TRY(up(m->curUR, m->h_curUR, nc, s));
    SIND_TRY(up(m->gstart, m->h_gstart, (size_t)B * 3073, s)); SIND_TRY(up(m->gidx, m->h_gidx, nc, s)); SIND_TRY(up(m->curTaken, m->h_curTaken, nc, s));
    sind::MatchArrays a{m->pose.p, m->nLast.p, m->nCur.p, m->x3Dw.p, m->lastFlags.p, m->lastOct.p, m->lastAng.p, m->lastDesc.p, m->curXY.p, m->curOct.p, m->curAng.p, m->curUR.p,
                        m->curDesc.p, m->gstart.p, m->gidx.p, m->curTaken.p, m->choice.p, m->minOwner.p, m->matchOfCur.p, m->nmatches.p, m->rounds.p};
    SIND_TRY(sind::launch_search_by_projection(p, a, B, s));
    HIP_TRY(hipMemcpyAsync(m->h_match.data(), m->matchOfCur.p, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_nm.data(), m->nmatches.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_rounds.data(), m->rounds.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    m->last_rounds = 0;
    for (int b = 0; b < B; b++) {
        std::memcpy(pairs[b].match_of_cur, &m->h_match[(size_t)b * cc], (size_t)pairs[b].n_cur * 4); *pairs[b].nmatches = m->h_nm[b];
        m->last_rounds = std::max(m->last_rounds, m->h_rounds[b]);
    }
    return SIND_OK;
}
int sind_match_last_rounds(sind_match* m) { return m ? m->last_rounds : SIND_E_ARG; }

}  // extern "C"

// ---- local-map search and relocalisation search (match_local.hip) ----
namespace {
struct PointsFrame {                                               // one frame of either call, the public structs flattened to one shape
    const float* Tcw; int n_points; const float* x3Dw; const float* normal; const float* max_dist; const float* min_dist; const uint8_t* flags; const float* angle; const uint8_t* desc;
    int n_cur; const float* cur_un_xy; const int* cur_octave; const float* cur_angle; const float* cur_u_right; const uint8_t* cur_desc; const int* grid_start; const int* grid_idx;
    const uint8_t* cur_taken;
    uint8_t* in_view; float* proj_xyr; int* level; float* view_cos; int* n_to_match; int* match_of_cur; int* nmatches;
};
}

static void cpy(void* d, const void* s, size_t n) { if (n) std::memcpy(d, s, n); }                  // empty frames may pass NULL arrays

static int run_points(sind_match* m, sind_match::PointSide& ps, const std::vector<PointsFrame>& fr, sind::LocalParams p, int reloc, const char* who) {
    const int B = (int)fr.size(), cp = ps.cap, cc = p.capCur;
    p.capPts = cp;
    p.logScaleFactor = (float)std::log((double)p.scale[1]);       // Frame.cc:71 with log as match_local.hip defines it
    bool wantFrustum = false;
    for (int b = 0; b < B; b++) {
        const PointsFrame& q = fr[b];
        if (q.n_points < 0 || q.n_points > cp || q.n_cur < 0 || q.n_cur > cc) { sind_set_error("%s: frame %d has %d points / %d keypoints, capacity %d / %d", who, b, q.n_points, q.n_cur, cp, cc); return SIND_E_CAPACITY; }
        if (!q.Tcw || !q.match_of_cur || !q.nmatches || !q.grid_start || (q.n_points && (!q.x3Dw || !q.max_dist || !q.min_dist || !q.flags || !q.desc || (reloc ? !q.angle : !q.normal))) ||
            (q.n_cur && (!q.cur_un_xy || !q.cur_octave || !q.cur_desc || !q.grid_idx || (reloc ? !q.cur_angle : !q.cur_u_right)))) { sind_set_error("%s: null array in frame %d", who, b); return SIND_E_ARG; }
        if (q.grid_start[0] != 0 || q.grid_start[3072] < 0 || q.grid_start[3072] > q.n_cur) { sind_set_error("%s: malformed grid of frame %d", who, b); return SIND_E_ARG; }
        for (int c = 0; c < 3072; c++) if (q.grid_start[c + 1] < q.grid_start[c]) { sind_set_error("%s: malformed grid of frame %d", who, b); return SIND_E_ARG; }
        for (int j = 0; j < q.grid_start[3072]; j++) if (q.grid_idx[j] < 0 || q.grid_idx[j] >= q.n_cur) { sind_set_error("%s: grid index outside the keypoints (frame %d)", who, b); return SIND_E_ARG; }
        wantFrustum = wantFrustum || q.in_view || q.proj_xyr || q.level || q.view_cos;
        sind::LocalPose& po = ps.h_pose[b]; cpy(po.Tcw, q.Tcw, sizeof(po.Tcw));
        for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)q.Tcw[4 * k + r] * (double)q.Tcw[4 * k + 3]; po.Ow[r] = (float)(s * -1.0); }   // -Rcw^T * tcw
        ps.h_nPts[b] = q.n_points; m->h_nCur[b] = q.n_cur;
        const size_t o = (size_t)b * cp, c0 = (size_t)b * cc, np = (size_t)q.n_points, nc = (size_t)q.n_cur;
        cpy(&ps.h_x3Dw[o * 3], q.x3Dw, np * 12); cpy(&ps.h_maxDist[o], q.max_dist, np * 4); cpy(&ps.h_minDist[o], q.min_dist, np * 4);
        cpy(&ps.h_desc[o * 32], q.desc, np * 32);
        if (reloc) { cpy(&ps.h_angle[o], q.angle, np * 4); for (size_t i = 0; i < np; i++) ps.h_flags[o + i] = q.flags[i] ? 3 : 0; }     // every assignment closes its keypoint (:1541)
        else { cpy(&ps.h_normal[o * 3], q.normal, np * 12); for (size_t i = 0; i < np; i++) ps.h_flags[o + i] = q.flags[i] & 3; }
        cpy(&m->h_curXY[c0 * 2], q.cur_un_xy, nc * 8); cpy(&m->h_curOct[c0], q.cur_octave, nc * 4); cpy(&m->h_curDesc[c0 * 32], q.cur_desc, nc * 32);
        if (reloc) cpy(&m->h_curAng[c0], q.cur_angle, nc * 4); else cpy(&m->h_curUR[c0], q.cur_u_right, nc * 4);
        cpy(&m->h_gstart[(size_t)b * 3073], q.grid_start, 3073 * 4); cpy(&m->h_gidx[c0], q.grid_idx, (size_t)q.grid_start[3072] * 4);
        if (q.cur_taken) cpy(&m->h_curTaken[c0], q.cur_taken, nc); else std::memset(&m->h_curTaken[c0], 0, nc);
    }
    SIND_TRY(m->curPack.alloc((size_t)m->maxB * cc));
    hipStream_t s = m->stream; const size_t np = (size_t)B * cp, nc = (size_t)B * cc;
    SIND_TRY(up(ps.pose, ps.h_pose, B, s)); SIND_TRY(up(ps.nPts, ps.h_nPts, B, s)); SIND_TRY(up(m->nCur, m->h_nCur, B, s)); SIND_TRY(up(ps.x3Dw, ps.h_x3Dw, np * 3, s));
    SIND_TRY(up(ps.maxDist, ps.h_maxDist, np, s)); SIND_TRY(up(ps.minDist, ps.h_minDist, np, s)); SIND_TRY(up(ps.flags, ps.h_flags, np, s));
    HIP_TRY(hipMemcpyAsync(ps.desc.p, ps.h_desc.data(), np * 32, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(m->curDesc.p, m->h_curDesc.data(), nc * 32, hipMemcpyHostToDevice, s));
    if (reloc) { SIND_TRY(up(ps.angle, ps.h_angle, np, s)); SIND_TRY(up(m->curAng, m->h_curAng, nc, s)); } else { SIND_TRY(up(ps.normal, ps.h_normal, np * 3, s)); SIND_TRY(up(m->curUR, m->h_curUR, nc, s)); }
    SIND_TRY(up(m->curXY, m->h_curXY, nc * 2, s)); SIND_TRY(up(m->curOct, m->h_curOct, nc, s));
    SIND_TRY(up(m->gstart, m->h_gstart, (size_t)B * 3073, s)); SIND_TRY(up(m->gidx, m->h_gidx, nc, s)); SIND_TRY(up(m->curTaken, m->h_curTaken, nc, s));
    HIP_TRY(hipMemsetAsync(ps.nToMatch.p, 0, (size_t)B * 4, s));
    sind::LocalArrays a{ps.pose.p, ps.nPts.p, m->nCur.p, ps.x3Dw.p, ps.normal.p, ps.maxDist.p, ps.minDist.p, ps.flags.p, ps.angle.p, ps.desc.p, m->curXY.p, m->curOct.p, m->curAng.p, m->curUR.p,
                        m->curDesc.p, m->gstart.p, m->gidx.p, m->curTaken.p, ps.inView.p, ps.projXYR.p, ps.level.p, ps.viewCos.p, ps.nToMatch.p, ps.choice.p, m->minOwner.p, m->curPack.p, m->matchOfCur.p,
                        m->nmatches.p, m->rounds.p};
    SIND_TRY(sind::launch_project_points(p, a, B, reloc, s));
    SIND_TRY(sind::launch_search_points(p, a, B, reloc, s));
    if (wantFrustum) {
        HIP_TRY(hipMemcpyAsync(ps.h_inView.data(), ps.inView.p, np, hipMemcpyDeviceToHost, s)); HIP_TRY(hipMemcpyAsync(ps.h_projXYR.data(), ps.projXYR.p, np * 12, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ps.h_level.data(), ps.level.p, np * 4, hipMemcpyDeviceToHost, s)); HIP_TRY(hipMemcpyAsync(ps.h_viewCos.data(), ps.viewCos.p, np * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(ps.h_nToMatch.data(), ps.nToMatch.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_match.data(), m->matchOfCur.p, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_nm.data(), m->nmatches.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_rounds.data(), m->rounds.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    m->last_rounds = 0;
    for (int b = 0; b < B; b++) {
        const PointsFrame& q = fr[b]; const size_t o = (size_t)b * cp, n = (size_t)q.n_points;
        if (q.in_view) cpy(q.in_view, &ps.h_inView[o], n); if (q.proj_xyr) cpy(q.proj_xyr, &ps.h_projXYR[o * 3], n * 12);
        if (q.level) cpy(q.level, &ps.h_level[o], n * 4); if (q.view_cos) cpy(q.view_cos, &ps.h_viewCos[o], n * 4);
        if (q.n_to_match) *q.n_to_match = ps.h_nToMatch[b];
        cpy(q.match_of_cur, &m->h_match[(size_t)b * cc], (size_t)q.n_cur * 4); *q.nmatches = m->h_nm[b];
        m->last_rounds = std::max(m->last_rounds, m->h_rounds[b]);
    }
    return SIND_OK;
}

static sind::LocalParams local_params(const sind_match* m, float th) {
    sind::LocalParams p{}; const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; p.bf = c.bf; std::memcpy(p.bounds, c.bounds, sizeof(p.bounds)); std::memcpy(p.scale, c.scale, sizeof(p.scale));
    p.nlevels = c.nlevels; p.capCur = c.capCur; p.th = th;
    return p;
}

extern "C" {

int sind_match_reserve_map_points(sind_match* m, int cap_points) {
    if (!m || cap_points < 1) { sind_set_error("sind_match_reserve_map_points: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return m->local.reserve((size_t)m->maxB, cap_points);
}

int sind_match_local_map(sind_match* m, const sind_match_local* frames, int B, float th, float nnratio, float viewing_cos_limit) {
    if (!m || !frames || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_local_map: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    if (!m->local.cap) { sind_set_error("sind_match_local_map: call sind_match_reserve_map_points first"); return SIND_E_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    sind::LocalParams p = local_params(m, th); p.nnratio = nnratio; p.viewCosLimit = viewing_cos_limit;
    std::vector<PointsFrame> fr(B);
    for (int b = 0; b < B; b++) {
        const sind_match_local& q = frames[b];
        fr[b] = PointsFrame{q.Tcw, q.n_points, q.x3Dw, q.normal, q.max_dist, q.min_dist, q.flags, nullptr, q.desc, q.n_cur, q.cur_un_xy, q.cur_octave, nullptr, q.cur_u_right, q.cur_desc,
                            q.grid_start, q.grid_idx, q.cur_taken, q.in_view, q.proj_xyr, q.level, q.view_cos, q.n_to_match, q.match_of_cur, q.nmatches};
    }
    return run_points(m, m->local, fr, p, 0, "sind_match_local_map");
}

int sind_match_by_projection_kf(sind_match* m, const sind_match_reloc* frames, int B, float th, int orb_dist, int check_orientation) {
    if (!m || !frames || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_by_projection_kf: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->reloc.cap) SIND_TRY(m->reloc.reserve((size_t)m->maxB, m->prm.capLast));
    sind::LocalParams p = local_params(m, th); p.orbDist = orb_dist; p.checkOrientation = check_orientation ? 1 : 0;
    std::vector<PointsFrame> fr(B);
    for (int b = 0; b < B; b++) {
        const sind_match_reloc& q = frames[b];
        fr[b] = PointsFrame{q.Tcw, q.n_points, q.x3Dw, nullptr, q.max_dist, q.min_dist, q.valid, q.kf_angle, q.desc, q.n_cur, q.cur_un_xy, q.cur_octave, q.cur_angle, nullptr, q.cur_desc,
                            q.grid_start, q.grid_idx, q.cur_taken, nullptr, nullptr, nullptr, nullptr, nullptr, q.match_of_cur, q.nmatches};
    }
    return run_points(m, m->reloc, fr, p, 1, "sind_match_by_projection_kf");
}

}  // extern "C"

// ---- vocabulary-guided searches (match_bow.hip) ----
static int sort_length(int n) { int p = 1; while (p < n) p <<= 1; return p; }

static int check_nodes(const int* node, int n) { for (int i = 0; i < n; i++) if (node[i] < -1) return 0; return 1; }

static sind::BowParams bow_params(const sind_match* m, int maxN) {
    sind::BowParams p{}; const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; std::memcpy(p.scale, c.scale, sizeof(p.scale)); p.capA = c.capLast; p.capB = c.capCur; p.sortLen = sort_length(maxN);
    return p;
}

static sind::BowArrays bow_arrays(sind_match* m) {
    sind_match::BowSide& w = m->bow;
    return sind::BowArrays{m->nLast.p, m->nCur.p, w.nodeA.p, w.nodeB.p, m->lastFlags.p, m->lastAng.p, m->lastDesc.p, m->curAng.p, m->curDesc.p, w.pose.p, w.lastXY.p, w.lastUR.p, m->curTaken.p,
                           m->curXY.p, m->curOct.p, m->curUR.p, w.sortedA.p, w.sortedB.p, w.segStart.p, w.nSeg.p, w.nValid.p, m->choice.p, m->matchOfCur.p, m->nmatches.p};
}

extern "C" {

int sind_match_by_bow(sind_match* m, const sind_match_bow* pairs, int B, float nnratio, int check_orientation) {
    const char* who = "sind_match_by_bow";
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("%s: bad arguments (B=%d, max %d)", who, B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int cl = std::min(m->prm.capLast, BOW_MAX_KEYS), cc = std::min(m->prm.capCur, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const sind_match_bow& q = pairs[b];
        if (q.n_kf < 0 || q.n_kf > cl || q.n_cur < 0 || q.n_cur > cc) { sind_set_error("%s: pair %d has %d / %d keypoints, capacity %d / %d", who, b, q.n_kf, q.n_cur, cl, cc); return SIND_E_CAPACITY; }
        if (!q.nmatches || (q.n_kf && (!q.kf_node || !q.kf_valid || !q.kf_angle || !q.kf_desc)) || (q.n_cur && (!q.cur_node || !q.cur_angle || !q.cur_desc || !q.match_of_cur))) {
            sind_set_error("%s: null array in pair %d", who, b); return SIND_E_ARG;
        }
        if (!check_nodes(q.kf_node, q.n_kf) || !check_nodes(q.cur_node, q.n_cur)) { sind_set_error("%s: node id below -1 in pair %d", who, b); return SIND_E_ARG; }
        maxN = std::max(maxN, std::max(q.n_kf, q.n_cur));
    }
    const size_t sl = m->prm.capLast, sc = m->prm.capCur;
    SIND_TRY(m->bow.reserve((size_t)m->maxB, sl, sc));
    sind_match::BowSide& w = m->bow;
    for (int b = 0; b < B; b++) {
        const sind_match_bow& q = pairs[b]; const size_t oa = b * sl, ob = b * sc, na = (size_t)q.n_kf, nb = (size_t)q.n_cur;
        m->h_nLast[b] = q.n_kf; m->h_nCur[b] = q.n_cur;
        cpy(&w.h_nodeA[oa], q.kf_node, na * 4); for (size_t i = 0; i < na; i++) m->h_lastFlags[oa + i] = q.kf_valid[i] ? 1 : 0;
        cpy(&m->h_lastAng[oa], q.kf_angle, na * 4); cpy(&m->h_lastDesc[oa * 32], q.kf_desc, na * 32);
        cpy(&w.h_nodeB[ob], q.cur_node, nb * 4); cpy(&m->h_curAng[ob], q.cur_angle, nb * 4); cpy(&m->h_curDesc[ob * 32], q.cur_desc, nb * 32);
    }
    hipStream_t s = m->stream; const size_t nl = (size_t)B * sl, nc = (size_t)B * sc;
    SIND_TRY(up(m->nLast, m->h_nLast, B, s)); SIND_TRY(up(m->nCur, m->h_nCur, B, s)); SIND_TRY(up(w.nodeA, w.h_nodeA, nl, s)); SIND_TRY(up(w.nodeB, w.h_nodeB, nc, s));
    SIND_TRY(up(m->lastFlags, m->h_lastFlags, nl, s)); SIND_TRY(up(m->lastAng, m->h_lastAng, nl, s)); SIND_TRY(up(m->curAng, m->h_curAng, nc, s));
    HIP_TRY(hipMemcpyAsync(m->lastDesc.p, m->h_lastDesc.data(), nl * 32, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(m->curDesc.p, m->h_curDesc.data(), nc * 32, hipMemcpyHostToDevice, s));
    sind::BowParams p = bow_params(m, maxN); p.nnratio = nnratio; p.checkOrientation = check_orientation ? 1 : 0;
    SIND_TRY(sind::launch_match_by_bow(p, bow_arrays(m), B, s));
    HIP_TRY(hipMemcpyAsync(m->h_match.data(), m->matchOfCur.p, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_nm.data(), m->nmatches.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) { cpy(pairs[b].match_of_cur, &m->h_match[b * sc], (size_t)pairs[b].n_cur * 4); *pairs[b].nmatches = m->h_nm[b]; }
    return SIND_OK;
}

int sind_match_for_triangulation(sind_match* m, const sind_match_tri* pairs, int B, int only_stereo, int check_orientation) {
    const char* who = "sind_match_for_triangulation";
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("%s: bad arguments (B=%d, max %d)", who, B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int cl = std::min(m->prm.capLast, BOW_MAX_KEYS), cc = std::min(m->prm.capCur, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const sind_match_tri& q = pairs[b];
        if (q.n1 < 0 || q.n1 > cl || q.n2 < 0 || q.n2 > cc) { sind_set_error("%s: pair %d has %d / %d keypoints, capacity %d / %d", who, b, q.n1, q.n2, cl, cc); return SIND_E_CAPACITY; }
        if (!q.Tcw2 || !q.Cw1 || !q.F12 || !q.nmatches || (q.n1 && (!q.node1 || !q.has_mp1 || !q.un_xy1 || !q.angle1 || !q.u_right1 || !q.desc1 || !q.match12)) ||
            (q.n2 && (!q.node2 || !q.has_mp2 || !q.un_xy2 || !q.octave2 || !q.angle2 || !q.u_right2 || !q.desc2))) { sind_set_error("%s: null array in pair %d", who, b); return SIND_E_ARG; }
        if (!check_nodes(q.node1, q.n1) || !check_nodes(q.node2, q.n2)) { sind_set_error("%s: node id below -1 in pair %d", who, b); return SIND_E_ARG; }
        for (int i = 0; i < q.n2; i++) if (q.octave2[i] < 0 || q.octave2[i] >= m->prm.nlevels) { sind_set_error("%s: octave %d outside [0,%d)", who, q.octave2[i], m->prm.nlevels); return SIND_E_ARG; }
        maxN = std::max(maxN, std::max(q.n1, q.n2));
    }
    const size_t sl = m->prm.capLast, sc = m->prm.capCur;
    SIND_TRY(m->bow.reserve((size_t)m->maxB, sl, sc));
    sind_match::BowSide& w = m->bow;
    for (int b = 0; b < B; b++) {
        const sind_match_tri& q = pairs[b]; const size_t oa = b * sl, ob = b * sc, na = (size_t)q.n1, nb = (size_t)q.n2;
        sind::TriPose& ps = w.h_pose[b]; cpy(ps.Tcw2, q.Tcw2, sizeof(ps.Tcw2)); cpy(ps.Cw1, q.Cw1, sizeof(ps.Cw1)); cpy(ps.F12, q.F12, sizeof(ps.F12));
        m->h_nLast[b] = q.n1; m->h_nCur[b] = q.n2;
        cpy(&w.h_nodeA[oa], q.node1, na * 4); for (size_t i = 0; i < na; i++) m->h_lastFlags[oa + i] = q.has_mp1[i] ? 1 : 0;
        cpy(&w.h_lastXY[oa * 2], q.un_xy1, na * 8); cpy(&m->h_lastAng[oa], q.angle1, na * 4); cpy(&w.h_lastUR[oa], q.u_right1, na * 4); cpy(&m->h_lastDesc[oa * 32], q.desc1, na * 32);
        cpy(&w.h_nodeB[ob], q.node2, nb * 4); for (size_t i = 0; i < nb; i++) m->h_curTaken[ob + i] = q.has_mp2[i] ? 1 : 0;
        cpy(&m->h_curXY[ob * 2], q.un_xy2, nb * 8); cpy(&m->h_curOct[ob], q.octave2, nb * 4); cpy(&m->h_curAng[ob], q.angle2, nb * 4); cpy(&m->h_curUR[ob], q.u_right2, nb * 4);
        cpy(&m->h_curDesc[ob * 32], q.desc2, nb * 32);
    }
    hipStream_t s = m->stream; const size_t nl = (size_t)B * sl, nc = (size_t)B * sc;
    SIND_TRY(up(w.pose, w.h_pose, B, s)); SIND_TRY(up(m->nLast, m->h_nLast, B, s)); SIND_TRY(up(m->nCur, m->h_nCur, B, s)); SIND_TRY(up(w.nodeA, w.h_nodeA, nl, s)); SIND_TRY(up(w.nodeB, w.h_nodeB, nc, s));
    SIND_TRY(up(m->lastFlags, m->h_lastFlags, nl, s)); SIND_TRY(up(w.lastXY, w.h_lastXY, nl * 2, s)); SIND_TRY(up(m->lastAng, m->h_lastAng, nl, s)); SIND_TRY(up(w.lastUR, w.h_lastUR, nl, s));
    SIND_TRY(up(m->curTaken, m->h_curTaken, nc, s)); SIND_TRY(up(m->curXY, m->h_curXY, nc * 2, s)); SIND_TRY(up(m->curOct, m->h_curOct, nc, s)); SIND_TRY(up(m->curAng, m->h_curAng, nc, s));
    SIND_TRY(up(m->curUR, m->h_curUR, nc, s));
    HIP_TRY(hipMemcpyAsync(m->lastDesc.p, m->h_lastDesc.data(), nl * 32, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(m->curDesc.p, m->h_curDesc.data(), nc * 32, hipMemcpyHostToDevice, s));
    sind::BowParams p = bow_params(m, maxN); p.onlyStereo = only_stereo ? 1 : 0; p.checkOrientation = check_orientation ? 1 : 0;
    SIND_TRY(sind::launch_match_for_triangulation(p, bow_arrays(m), B, s));
    HIP_TRY(hipMemcpyAsync(w.h_match12.data(), m->choice.p, nl * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_nm.data(), m->nmatches.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) { cpy(pairs[b].match12, &w.h_match12[b * sl], (size_t)pairs[b].n1 * 4); *pairs[b].nmatches = m->h_nm[b]; }
    return SIND_OK;
}

}  // extern "C"
