// C ABI: independent projections into a key frame, Fuse and SearchBySim3 (include/sind_hip.h, "sind_match_fuse", "sind_match_by_sim3"; match_fuse.hip).
#include "match_handle.hpp"

namespace {
// ---- independent projections into a key frame (match_fuse.hip) ----
sind::KfParams kf_params(const sind_match* m, float th, int thDist, int capP, int capK) {
    sind::KfParams p{}; const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; p.bf = c.bf; kf_bounds(c.bounds, p.bounds, p.gridInv); std::memcpy(p.scale, c.scale, sizeof(p.scale));
    for (int l = 0; l < c.nlevels; l++) p.invSigma2[l] = 1.0f / (c.scale[l] * c.scale[l]);       // mvLevelSigma2, mvInvLevelSigma2 (src/ORBextractor.cc:425-431)
    p.nlevels = c.nlevels; p.th = th; p.thDist = thDist; p.capPts = capP; p.capKeys = capK;
    p.logScaleFactor = (float)std::log((double)p.scale[1]);
    return p;
}

struct KfPoints { int n; const float* x3Dw; const float* normal; const float* maxDist; const float* minDist; const uint8_t* valid; const uint8_t* desc; };

int check_kf(const char* who, int b, bool otherNull, const KfPoints& pt, int capP, bool normals, const Keys& k, int capK, int useK, int nlevels) {
    const Keys pts{pt.n, nullptr, nullptr, nullptr, nullptr, pt.desc, nullptr, nullptr, nullptr, nullptr};
    SIND_TRY(check(who, b, otherNull || (pt.n && (!pt.x3Dw || !pt.maxDist || !pt.minDist || !pt.valid || (normals && !pt.normal))), pts, capP, 0, k, capK, useK));
    return check_octaves(who, b, k, nlevels);
}

// item q of a KfSide: its points and the keypoints an item searches (its own, or for sind_match_by_sim3 those the other side of the pair searches)
void stage_kf(sind_match::KfSide& w, int q, const KfPoints& pt, const Keys& k) {
    const size_t o = (size_t)q * w.capP, n = (size_t)pt.n, co = (size_t)q * w.capK;
    w.nP.h[q] = pt.n; put(w.x3Dw, o * 3, pt.x3Dw, n * 3); if (pt.normal) put(w.normal, o * 3, pt.normal, n * 3); put(w.maxDist, o, pt.maxDist, n); put(w.minDist, o, pt.minDist, n);
    put(w.valid, o, pt.valid, n); put(w.ptDesc, o * DESC_WORDS, pt.desc, n * DESC_WORDS);
    put(w.keyDesc, co * DESC_WORDS, k.desc, (size_t)k.n * DESC_WORDS);
    put(w.gridStart, (size_t)q * (GRID_CELLS + 1), k.gridStart, GRID_CELLS + 1); put(w.gridIdx, co, k.gridIdx, (size_t)k.gridStart[GRID_CELLS]);
    for (int c = 0; c < k.n; c++) { float4 r; r.x = k.xy[2 * c]; r.y = k.xy[2 * c + 1]; r.z = k.uRight ? k.uRight[c] : 0.f; int oc = k.octave[c]; std::memcpy(&r.w, &oc, 4); w.pack.h[co + c] = r; }
}

int upload_kf(sind_match::KfSide& w, int items, bool normals, hipStream_t s) {
    const size_t np = (size_t)items * w.capP, nk = (size_t)items * w.capK;
    SIND_TRY(w.pose.up(items, s)); SIND_TRY(w.nP.up(items, s)); SIND_TRY(w.x3Dw.up(np * 3, s)); if (normals) SIND_TRY(w.normal.up(np * 3, s));
    SIND_TRY(w.maxDist.up(np, s)); SIND_TRY(w.minDist.up(np, s)); SIND_TRY(w.valid.up(np, s)); SIND_TRY(w.ptDesc.up(np * DESC_WORDS, s)); SIND_TRY(w.keyDesc.up(nk * DESC_WORDS, s));
    SIND_TRY(w.gridStart.up((size_t)items * (GRID_CELLS + 1), s)); SIND_TRY(w.gridIdx.up(nk, s)); SIND_TRY(w.pack.up(nk, s));
    HIP_TRY(hipMemsetAsync(w.count.d.p, 0, (size_t)items * sizeof(int), s));
    return SIND_OK;
}

sind::KfArrays kf_arrays(sind_match::KfSide& w) {
    return sind::KfArrays{w.pose.d.p, w.nP.d.p, w.x3Dw.d.p, w.normal.d.p, w.maxDist.d.p, w.minDist.d.p, w.valid.d.p, w.ptDesc.d.p, w.pack.d.p, w.keyDesc.d.p, w.gridStart.d.p, w.gridIdx.d.p,
                          w.bestIdx.d.p, w.bestDist.d.p, w.count.d.p, w.match12.d.p};
}

KfPoints points_of(const sind_match_sim3_side& q) { return KfPoints{q.n, q.x3Dw, nullptr, q.max_dist, q.min_dist, q.valid, q.mp_desc}; }
Keys keys_of(const sind_match_sim3_side& q) { return Keys{q.n, q.un_xy, q.octave, nullptr, nullptr, q.kf_desc, nullptr, q.grid_start, q.grid_idx, nullptr}; }
}  // namespace

extern "C" {

int sind_match_fuse(sind_match* m, const sind_match_fuse_item* items, int B, float th, int sim3) {
    const char* who = "sind_match_fuse: item";
    if (!m || !items || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_fuse: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    if (!m->local.cap) { sind_set_error("sind_match_fuse: call sind_match_reserve_map_points first"); return SIND_E_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    const int cp = m->local.cap, ck = m->cur.cap, useK = K_XY | K_OCTAVE | K_GRID | (sim3 ? 0 : K_URIGHT);
    auto points = [](const sind_match_fuse_item& q) { return KfPoints{q.n_points, q.x3Dw, q.normal, q.max_dist, q.min_dist, q.valid, q.desc}; };
    auto keys = [sim3](const sind_match_fuse_item& q) { return Keys{q.n_kf, q.kf_un_xy, q.kf_octave, nullptr, sim3 ? nullptr : q.kf_u_right, q.kf_desc, nullptr, q.grid_start, q.grid_idx, nullptr}; };
    for (int b = 0; b < B; b++) {
        const sind_match_fuse_item& q = items[b];
        SIND_TRY(check_kf(who, b, !q.Tcw || !q.nfused || (q.n_points && (!q.best_idx || !q.best_dist)), points(q), cp, true, keys(q), ck, useK, m->prm.nlevels));
    }
    sind_match::KfSide& w = m->fuse;
    SIND_TRY(w.reserve((size_t)m->maxB, cp, ck));
    for (int b = 0; b < B; b++) {
        const sind_match_fuse_item& q = items[b];
        sind::KfPose& ps = w.pose.h[b];
        if (sim3) decompose_scw(q.Tcw, ps.T); else cpy(ps.T, q.Tcw, sizeof(ps.T));
        camera_centre(ps.T, ps.Ow);
        stage_kf(w, b, points(q), keys(q));
    }
    hipStream_t s = m->stream; const size_t np = (size_t)B * cp;
    SIND_TRY(upload_kf(w, B, true, s));
    SIND_TRY(sind::launch_search_kf(kf_params(m, th, 50, cp, ck), kf_arrays(w), B, sim3 ? sind::KF_FUSE_SIM3 : sind::KF_FUSE, s));
    SIND_TRY(w.bestIdx.down(np, s)); SIND_TRY(w.bestDist.down(np, s)); SIND_TRY(w.count.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        const sind_match_fuse_item& q = items[b]; const size_t o = (size_t)b * cp, n = (size_t)q.n_points;
        cpy(q.best_idx, &w.bestIdx.h[o], n * sizeof(int)); cpy(q.best_dist, &w.bestDist.h[o], n * sizeof(int)); *q.nfused = w.count.h[b];
    }
    return SIND_OK;
}

int sind_match_by_sim3(sind_match* m, const sind_match_sim3_pair* pairs, int B, float th) {
    const char* who = "sind_match_by_sim3: pair";
    if (!m || !pairs || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_by_sim3: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int cs = std::min(m->last.cap, m->cur.cap), useK = K_XY | K_OCTAVE | K_GRID;
    for (int b = 0; b < B; b++) {
        const sind_match_sim3_pair& q = pairs[b];
        const bool otherNull = !q.T1w || !q.T2w || !q.R12 || !q.t12 || !q.nfound || (q.side1.n && !q.match12);
        if (q.side1.n < 0 || q.side1.n > cs || q.side2.n < 0 || q.side2.n > cs) { sind_set_error("%s %d has %d / %d slots, capacity %d", who, b, q.side1.n, q.side2.n, cs); return SIND_E_CAPACITY; }
        SIND_TRY(check_kf(who, b, otherNull, points_of(q.side1), cs, false, keys_of(q.side1), cs, useK, m->prm.nlevels));
        SIND_TRY(check_kf(who, b, otherNull, points_of(q.side2), cs, false, keys_of(q.side2), cs, useK, m->prm.nlevels));
    }
    sind_match::KfSide& w = m->sim3;
    SIND_TRY(w.reserve(2 * (size_t)m->maxB, cs, cs));
    for (int b = 0; b < B; b++) {
        const sind_match_sim3_pair& q = pairs[b];
        sind::KfPose& p1 = w.pose.h[2 * b]; sind::KfPose& p2 = w.pose.h[2 * b + 1];
        cpy(p1.T, q.T1w, sizeof(p1.T)); cpy(p2.T, q.T2w, sizeof(p2.T));
        const float ia = (float)(1.0 / (double)q.s12);                                                   // :1119-1121; match_local.hip (5), (7)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) { p2.T2[4 * r + c] = q.s12 * q.R12[3 * r + c]; p1.T2[4 * r + c] = ia * q.R12[3 * c + r]; }
            p2.T2[4 * r + 3] = q.t12[r];
        }
        for (int r = 0; r < 3; r++) { const float t = p1.T2[4 * r] * q.t12[0] + p1.T2[4 * r + 1] * q.t12[1] + p1.T2[4 * r + 2] * q.t12[2]; p1.T2[4 * r + 3] = (float)((double)t * -1.0); }
        for (int k = 0; k < 3; k++) p1.Ow[k] = p2.Ow[k] = 0.f;                                           // not read: the distance is |p3Dc|
        stage_kf(w, 2 * b, points_of(q.side1), keys_of(q.side1)); stage_kf(w, 2 * b + 1, points_of(q.side2), keys_of(q.side2));
    }
    hipStream_t s = m->stream;
    SIND_TRY(upload_kf(w, 2 * B, false, s));
    const sind::KfParams p = kf_params(m, th, 100, cs, cs); const sind::KfArrays a = kf_arrays(w);
    SIND_TRY(sind::launch_search_kf(p, a, 2 * B, sind::KF_BY_SIM3, s));
    SIND_TRY(sind::launch_sim3_agree(p, a, B, s));
    SIND_TRY(w.match12.down((size_t)B * cs, s)); SIND_TRY(w.count.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) { const sind_match_sim3_pair& q = pairs[b]; cpy(q.match12, &w.match12.h[(size_t)b * cs], (size_t)q.side1.n * sizeof(int)); *q.nfound = w.count.h[b]; }
    return SIND_OK;
}

}  // extern "C"
