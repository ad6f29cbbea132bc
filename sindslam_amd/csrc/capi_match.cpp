// C ABI: the matcher handle and its projection searches (include/sind_hip.h, "sind_match_*"); match_handle.hpp names the files of the other families.
#include "match_handle.hpp"

namespace {
// CurrentFrame / LastFrame pose algebra of ORBmatcher.cc:1338-1349 (cv::gemm semantics: A*b+c without transposition = FP32 row
// product then FP64 alpha/beta; -A^T*b = FP64 accumulation)
void forward_backward(const float* Tc, const float* Tl, float mb, bool mono, int& fwd, int& bwd) {
    float twc[3], tlc[3];
    for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)Tc[4 * k + r] * (double)Tc[4 * k + 3]; twc[r] = (float)(s * -1.0); }
    for (int r = 0; r < 3; r++) { const float t = Tl[4 * r] * twc[0] + Tl[4 * r + 1] * twc[1] + Tl[4 * r + 2] * twc[2]; tlc[r] = (float)((double)t * 1.0 + (double)Tl[4 * r + 3] * 1.0); }
    fwd = tlc[2] > mb && !mono; bwd = -tlc[2] > mb && !mono;
}

// ---- local-map search, relocalisation search (match_local.hip) and SearchByProjection(pKF, Scw) (mode 2: projection of match_fuse.hip) ----
struct PointsFrame {                                               // one frame of either call, the public structs flattened to one shape
    const float* Tcw; int n_points; const float* x3Dw; const float* normal; const float* max_dist; const float* min_dist; const uint8_t* flags; const float* angle; const uint8_t* desc;
    Keys cur;
    uint8_t* in_view; float* proj_xyr; int* level; float* view_cos; int* n_to_match; int* match_of_cur; int* nmatches;
};

int run_points(sind_match* m, sind_match::PointSide& ps, const std::vector<PointsFrame>& fr, sind::LocalParams p, int mode, const char* who) {
    const bool reloc = mode == 1, closing = mode != 0, normals = mode != 1;                  // modes 1 and 2: every assignment closes its keypoint (:1541, :396)
    const int B = (int)fr.size(), cp = ps.cap, use = K_XY | K_OCTAVE | K_FLAGS | K_GRID | (mode == 1 ? K_ANGLE : mode == 0 ? K_URIGHT : 0);
    Side& c = m->cur;
    p.capPts = cp;
    p.logScaleFactor = (float)std::log((double)p.scale[1]);       // Frame.cc:71 with log as match_local.hip defines it
    bool wantFrustum = false;
    for (int b = 0; b < B; b++) {
        const PointsFrame& q = fr[b];
        const Keys pts{q.n_points, nullptr, nullptr, reloc ? q.angle : nullptr, nullptr, q.desc, nullptr, nullptr, nullptr, nullptr};      // as far as check() goes
        SIND_TRY(check(who, b, !q.Tcw || !q.match_of_cur || !q.nmatches || (q.n_points && (!q.x3Dw || !q.max_dist || !q.min_dist || !q.flags || (normals && !q.normal))), pts, cp, reloc ? K_ANGLE : 0,
                       q.cur, c.cap, use));
        if (mode == 2) SIND_TRY(check_octaves(who, b, q.cur, p.nlevels));
        wantFrustum = wantFrustum || q.in_view || q.proj_xyr || q.level || q.view_cos;
        sind::LocalPose& po = ps.pose.h[b]; cpy(po.Tcw, q.Tcw, sizeof(po.Tcw));
        camera_centre(q.Tcw, po.Ow);
        const size_t o = (size_t)b * cp, n = (size_t)q.n_points;
        ps.n.h[b] = q.n_points; put(ps.x3Dw, o * 3, q.x3Dw, n * 3); put(ps.maxDist, o, q.max_dist, n); put(ps.minDist, o, q.min_dist, n); put(ps.desc, o * DESC_WORDS, q.desc, n * DESC_WORDS);
        if (reloc) put(ps.angle, o, q.angle, n);
        if (normals) put(ps.normal, o * 3, q.normal, n * 3);
        for (size_t i = 0; i < n; i++) ps.flags.h[o + i] = closing ? (q.flags[i] ? 3 : 0) : q.flags[i] & 3;
        c.stage(b, q.cur, use);
        m->out[b] = {q.match_of_cur, q.cur.n, q.nmatches};
    }
    SIND_TRY(m->curPack.alloc((size_t)m->maxB * c.cap));
    hipStream_t s = m->stream; const size_t np = (size_t)B * cp;
    SIND_TRY(ps.pose.up(B, s)); SIND_TRY(ps.n.up(B, s)); SIND_TRY(ps.x3Dw.up(np * 3, s)); SIND_TRY(ps.maxDist.up(np, s)); SIND_TRY(ps.minDist.up(np, s)); SIND_TRY(ps.flags.up(np, s));
    SIND_TRY(ps.desc.up(np * DESC_WORDS, s)); if (reloc) SIND_TRY(ps.angle.up(np, s)); if (normals) SIND_TRY(ps.normal.up(np * 3, s)); SIND_TRY(c.upload(B, use, s));
    HIP_TRY(hipMemsetAsync(ps.nToMatch.d.p, 0, (size_t)B * 4, s));
    sind::LocalArrays a{ps.pose.d.p, ps.n.d.p, c.n.d.p, ps.x3Dw.d.p, ps.normal.d.p, ps.maxDist.d.p, ps.minDist.d.p, ps.flags.d.p, ps.angle.d.p, ps.desc.d.p, c.xy.d.p, c.octave.d.p, c.angle.d.p,
                        c.uRight.d.p, c.desc.d.p, c.gridStart.d.p, c.gridIdx.d.p, c.flags.d.p, ps.inView.d.p, ps.projXYR.d.p, ps.level.d.p, ps.viewCos.d.p, ps.nToMatch.d.p, ps.choice.p,
                        m->minOwner.p, m->curPack.p, m->matchOfCur.d.p, m->nmatches.d.p, m->rounds.d.p};
    SIND_TRY(mode == 2 ? sind::launch_project_kf(p, a, B, s) : sind::launch_project_points(p, a, B, mode, s));
    SIND_TRY(sind::launch_search_points(p, a, B, mode, s));
    if (wantFrustum) { SIND_TRY(ps.inView.down(np, s)); SIND_TRY(ps.projXYR.down(np * 3, s)); SIND_TRY(ps.level.down(np, s)); SIND_TRY(ps.viewCos.down(np, s)); }
    SIND_TRY(ps.nToMatch.down(B, s));
    SIND_TRY(finish(m, B, m->matchOfCur, c.cap, true));
    for (int b = 0; b < B; b++) {
        const PointsFrame& q = fr[b]; const size_t o = (size_t)b * cp, n = (size_t)q.n_points;
        if (q.in_view) cpy(q.in_view, &ps.inView.h[o], n); if (q.proj_xyr) cpy(q.proj_xyr, &ps.projXYR.h[o * 3], n * 12);
        if (q.level) cpy(q.level, &ps.level.h[o], n * 4); if (q.view_cos) cpy(q.view_cos, &ps.viewCos.h[o], n * 4);
        if (q.n_to_match) *q.n_to_match = ps.nToMatch.h[b];
    }
    return SIND_OK;
}

sind::LocalParams local_params(const sind_match* m, float th) {
    sind::LocalParams p{}; const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; p.bf = c.bf; std::memcpy(p.bounds, c.bounds, sizeof(p.bounds)); std::memcpy(p.scale, c.scale, sizeof(p.scale));
    p.nlevels = c.nlevels; p.capCur = c.capCur; p.th = th;
    return p;
}
}  // namespace

// ---- the C ABI ----
extern "C" {

int sind_match_create(const sind_match_config* c, sind_match** out) {
    if (!c || !out || c->cap_last < 1 || c->cap_cur < 1 || c->max_batch < 1 || c->nlevels < 1 || c->nlevels > 16 || !(c->fx > 0)) { sind_set_error("sind_match_create: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    sind_match* m = new sind_match(); m->device = c->device; m->maxB = c->max_batch;
    sind::MatchParams& p = m->prm; p.fx = c->fx; p.fy = c->fy; p.cx = c->cx; p.cy = c->cy; p.bf = c->bf; std::memcpy(p.bounds, c->bounds, sizeof(p.bounds));
    for (int i = 0; i < 16; i++) p.scale[i] = i < c->nlevels ? c->scale_factors[i] : 0.f;
    p.nlevels = c->nlevels; p.capLast = c->cap_last; p.capCur = c->cap_cur; m->mb = c->bf / c->fx;                 // Frame.cc:167 mb = mbf / fx
    const size_t B = c->max_batch, nl = B * c->cap_last, nc = B * c->cap_cur;
    Side& l = m->last; Side& k = m->cur; l.cap = c->cap_last; k.cap = c->cap_cur;
    int r = SIND_OK;
    if ((r = m->pose.alloc(B)) || (r = m->x3Dw.alloc(nl * 3)) || (r = l.n.alloc(B)) || (r = l.octave.alloc(nl)) || (r = l.angle.alloc(nl)) || (r = l.flags.alloc(nl)) || (r = l.desc.alloc(nl * DESC_WORDS)) ||
        (r = k.n.alloc(B)) || (r = k.xy.alloc(nc * 2)) || (r = k.octave.alloc(nc)) || (r = k.angle.alloc(nc)) || (r = k.uRight.alloc(nc)) || (r = k.flags.alloc(nc)) || (r = k.desc.alloc(nc * DESC_WORDS)) ||
        (r = k.gridStart.alloc(B * (GRID_CELLS + 1))) || (r = k.gridIdx.alloc(nc)) || (r = m->matchOfCur.alloc(nc)) || (r = m->nmatches.alloc(B)) || (r = m->rounds.alloc(B)) || (r = m->choice.d.alloc(nl)) ||
        (r = m->minOwner.alloc(nc))) { delete m; return r; }
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; sind_set_error("sind_match_create: stream creation failed"); return SIND_E_HIP; }
    m->out.resize(B);
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
    const int useLast = K_OCTAVE | K_ANGLE, useCur = K_XY | K_OCTAVE | K_ANGLE | K_URIGHT | K_FLAGS | K_GRID;      // last.flags is put together here
    Side& l = m->last; Side& c = m->cur;
    for (int b = 0; b < B; b++) {
        const sind_match_pair& q = pairs[b];
        const Keys last{q.n_last, nullptr, q.last_octave, q.last_angle, nullptr, q.last_desc, nullptr, nullptr, nullptr, nullptr};
        const Keys cur{q.n_cur, q.cur_un_xy, q.cur_octave, q.cur_angle, q.cur_u_right, q.cur_desc, q.cur_taken, q.grid_start, q.grid_idx, nullptr};
        SIND_TRY(check("sind_match_by_projection: pair", b, !q.Tcw_cur || !q.Tcw_last || !q.match_of_cur || !q.nmatches || (q.n_last && (!q.x3Dw || !q.last_valid || !q.last_has_obs)), last, l.cap, useLast,
                       cur, c.cap, useCur));
        const size_t o = (size_t)b * l.cap;
        for (int i = 0; i < q.n_last; i++) {
            if (q.last_octave[i] < 0 || q.last_octave[i] >= p.nlevels) { sind_set_error("sind_match_by_projection: octave %d outside [0,%d)", q.last_octave[i], p.nlevels); return SIND_E_ARG; }
            l.flags.h[o + i] = (uint8_t)((q.last_valid[i] ? 1 : 0) | (q.last_has_obs[i] ? 2 : 0));
        }
        sind::MatchPose& ps = m->pose.h[b]; std::memcpy(ps.Tcw, q.Tcw_cur, sizeof(ps.Tcw));
        forward_backward(q.Tcw_cur, q.Tcw_last, m->mb, mono != 0, ps.forward, ps.backward);
        put(m->x3Dw, o * 3, q.x3Dw, (size_t)q.n_last * 3); l.stage(b, last, useLast); c.stage(b, cur, useCur);
        m->out[b] = {q.match_of_cur, q.n_cur, q.nmatches};
    }
    hipStream_t s = m->stream; const size_t nl = (size_t)B * l.cap;
    SIND_TRY(m->pose.up(B, s)); SIND_TRY(m->x3Dw.up(nl * 3, s)); SIND_TRY(l.flags.up(nl, s)); SIND_TRY(l.upload(B, useLast, s)); SIND_TRY(c.upload(B, useCur, s));
    sind::MatchArrays a{m->pose.d.p, l.n.d.p, c.n.d.p, m->x3Dw.d.p, l.flags.d.p, l.octave.d.p, l.angle.d.p, l.desc.d.p, c.xy.d.p, c.octave.d.p, c.angle.d.p, c.uRight.d.p,
                        c.desc.d.p, c.gridStart.d.p, c.gridIdx.d.p, c.flags.d.p, m->choice.d.p, m->minOwner.p, m->matchOfCur.d.p, m->nmatches.d.p, m->rounds.d.p};
    SIND_TRY(sind::launch_search_by_projection(p, a, B, s));
    return finish(m, B, m->matchOfCur, m->cur.cap, true);
}
int sind_match_last_rounds(sind_match* m) { return m ? m->last_rounds : SIND_E_ARG; }

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
        fr[b] = PointsFrame{q.Tcw, q.n_points, q.x3Dw, q.normal, q.max_dist, q.min_dist, q.flags, nullptr, q.desc,
                            Keys{q.n_cur, q.cur_un_xy, q.cur_octave, nullptr, q.cur_u_right, q.cur_desc, q.cur_taken, q.grid_start, q.grid_idx, nullptr},
                            q.in_view, q.proj_xyr, q.level, q.view_cos, q.n_to_match, q.match_of_cur, q.nmatches};
    }
    return run_points(m, m->local, fr, p, 0, "sind_match_local_map: frame");
}

int sind_match_by_projection_kf(sind_match* m, const sind_match_reloc* frames, int B, float th, int orb_dist, int check_orientation) {
    if (!m || !frames || B < 1 || B > m->maxB || !(th > 0)) { sind_set_error("sind_match_by_projection_kf: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->reloc.cap) SIND_TRY(m->reloc.reserve((size_t)m->maxB, m->prm.capLast));
    sind::LocalParams p = local_params(m, th); p.orbDist = orb_dist; p.checkOrientation = check_orientation ? 1 : 0;
    std::vector<PointsFrame> fr(B);
    for (int b = 0; b < B; b++) {
        const sind_match_reloc& q = frames[b];
        fr[b] = PointsFrame{q.Tcw, q.n_points, q.x3Dw, nullptr, q.max_dist, q.min_dist, q.valid, q.kf_angle, q.desc,
                            Keys{q.n_cur, q.cur_un_xy, q.cur_octave, q.cur_angle, nullptr, q.cur_desc, q.cur_taken, q.grid_start, q.grid_idx, nullptr},
                            nullptr, nullptr, nullptr, nullptr, nullptr, q.match_of_cur, q.nmatches};
    }
    return run_points(m, m->reloc, fr, p, 1, "sind_match_by_projection_kf: frame");
}

int sind_match_by_projection_sim3(sind_match* m, const sind_match_proj_sim3* items, int B, int th) {
    if (!m || !items || B < 1 || B > m->maxB || th < 1) { sind_set_error("sind_match_by_projection_sim3: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    if (!m->local.cap) { sind_set_error("sind_match_by_projection_sim3: call sind_match_reserve_map_points first"); return SIND_E_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    sind::LocalParams p = local_params(m, (float)th); p.orbDist = 50; p.checkOrientation = 0;              // TH_LOW
    kf_bounds(m->prm.bounds, p.bounds, p.gridInv);
    std::vector<PointsFrame> fr(B); std::vector<float> T((size_t)B * 12);
    for (int b = 0; b < B; b++) {
        const sind_match_proj_sim3& q = items[b];
        if (q.Scw) decompose_scw(q.Scw, &T[(size_t)b * 12]);
        fr[b] = PointsFrame{q.Scw ? &T[(size_t)b * 12] : nullptr, q.n_points, q.x3Dw, q.normal, q.max_dist, q.min_dist, q.valid, nullptr, q.desc,
                            Keys{q.n_kf, q.kf_un_xy, q.kf_octave, nullptr, nullptr, q.kf_desc, q.kf_taken, q.grid_start, q.grid_idx, nullptr},
                            nullptr, nullptr, nullptr, nullptr, nullptr, q.match_of_kf, q.nmatches};
    }
    return run_points(m, m->local, fr, p, 2, "sind_match_by_projection_sim3: item");
}

}  // extern "C"
