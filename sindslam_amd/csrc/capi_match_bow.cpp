// C ABI: the vocabulary-guided searches SearchByBoW (frame and key frame) and SearchForTriangulation (include/sind_hip.h, "sind_match_by_bow*", "sind_match_for_triangulation"; match_bow.hip).
#include "match_handle.hpp"

namespace {
// a pair of each search: its two sides, a NULL among its other arrays, where its matches go, and the pair geometry only the triangulation has
Keys side_a(const sind_match_bow& q) { return Keys{q.n_kf, nullptr, nullptr, q.kf_angle, nullptr, q.kf_desc, q.kf_valid, nullptr, nullptr, q.kf_node}; }
Keys side_b(const sind_match_bow& q) { return Keys{q.n_cur, nullptr, nullptr, q.cur_angle, nullptr, q.cur_desc, nullptr, nullptr, nullptr, q.cur_node}; }
Keys side_a(const sind_match_bow_kf& q) { return Keys{q.n1, nullptr, nullptr, q.angle1, nullptr, q.desc1, q.valid1, nullptr, nullptr, q.node1}; }
Keys side_b(const sind_match_bow_kf& q) { return Keys{q.n2, nullptr, nullptr, q.angle2, nullptr, q.desc2, q.valid2, nullptr, nullptr, q.node2}; }
Keys side_a(const sind_match_tri& q) { return Keys{q.n1, q.un_xy1, nullptr, q.angle1, q.u_right1, q.desc1, q.has_mp1, nullptr, nullptr, q.node1}; }
Keys side_b(const sind_match_tri& q) { return Keys{q.n2, q.un_xy2, q.octave2, q.angle2, q.u_right2, q.desc2, q.has_mp2, nullptr, nullptr, q.node2}; }

bool other_null(const sind_match_bow& q) { return !q.nmatches || (q.n_cur && !q.match_of_cur) || (q.n_kf && !q.kf_valid); }
bool other_null(const sind_match_bow_kf& q) { return !q.nmatches || (q.n1 && (!q.match12 || !q.valid1)) || (q.n2 && !q.valid2); }
bool other_null(const sind_match_tri& q) { return !q.Tcw2 || !q.Cw1 || !q.F12 || !q.nmatches || (q.n1 && (!q.match12 || !q.has_mp1)) || (q.n2 && !q.has_mp2); }
sind_match::Result result_of(const sind_match_bow& q) { return {q.match_of_cur, q.n_cur, q.nmatches}; }
sind_match::Result result_of(const sind_match_bow_kf& q) { return {q.match12, q.n1, q.nmatches}; }
sind_match::Result result_of(const sind_match_tri& q) { return {q.match12, q.n1, q.nmatches}; }
template <class Pair> void stage_pose(const Pair&, sind::TriPose&) {}
void stage_pose(const sind_match_tri& q, sind::TriPose& ps) { cpy(ps.Tcw2, q.Tcw2, sizeof(ps.Tcw2)); cpy(ps.Cw1, q.Cw1, sizeof(ps.Cw1)); cpy(ps.F12, q.F12, sizeof(ps.F12)); }

// the rest of what differs.  byLast: the matches are match12 [n1], from choice with stride cap_last; else match_of_cur [n_cur], from matchOfCur with stride cap_cur
struct BowKind { const char* fn; const char* who; int useA, useB; bool byLast, tri; int (*launch)(const sind::BowParams&, const sind::BowArrays&, int, hipStream_t); };

sind::BowArrays bow_arrays(sind_match* m) {
    Side& l = m->last; Side& c = m->cur; sind_match::BowSide& w = m->bow;
    return sind::BowArrays{l.n.d.p, c.n.d.p, l.node.d.p, c.node.d.p, l.flags.d.p, l.angle.d.p, l.desc.d.p, c.angle.d.p, c.desc.d.p, w.pose.d.p, l.xy.d.p, l.uRight.d.p, c.flags.d.p,
                           c.xy.d.p, c.octave.d.p, c.uRight.d.p, w.sortedA.p, w.sortedB.p, w.segStart.p, w.nSeg.p, w.nValid.p, m->choice.d.p, m->matchOfCur.d.p, m->nmatches.d.p};
}

// p: the call's own parameters; the handle's and the sort length are added here
template <class Pair> int run_bow(sind_match* m, const BowKind& k, const Pair* pairs, int B, sind::BowParams p) {
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("%s: bad arguments (B=%d, max %d)", k.fn, B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int cl = std::min(m->last.cap, BOW_MAX_KEYS), cc = std::min(m->cur.cap, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const Keys qa = side_a(pairs[b]), qb = side_b(pairs[b]);
        SIND_TRY(check(k.who, b, other_null(pairs[b]), qa, cl, k.useA, qb, cc, k.useB));
        if (k.useB & K_OCTAVE) SIND_TRY(check_octaves(k.who, b, qb, m->prm.nlevels));
        maxN = std::max(maxN, std::max(qa.n, qb.n));
    }
    SIND_TRY(m->reserve_bow());
    for (int b = 0; b < B; b++) {
        stage_pose(pairs[b], m->bow.pose.h[b]);
        m->last.stage(b, side_a(pairs[b]), k.useA); m->cur.stage(b, side_b(pairs[b]), k.useB); m->out[b] = result_of(pairs[b]);
    }
    hipStream_t s = m->stream;
    if (k.tri) SIND_TRY(m->bow.pose.up(B, s));
    SIND_TRY(m->last.upload(B, k.useA, s)); SIND_TRY(m->cur.upload(B, k.useB, s));
    const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; std::memcpy(p.scale, c.scale, sizeof(p.scale)); p.capA = c.capLast; p.capB = c.capCur;
    p.sortLen = 1; while (p.sortLen < maxN) p.sortLen <<= 1;
    SIND_TRY(k.launch(p, bow_arrays(m), B, s));
    return k.byLast ? finish(m, B, m->choice, m->last.cap, false) : finish(m, B, m->matchOfCur, m->cur.cap, false);
}
}  // namespace

extern "C" {

int sind_match_by_bow(sind_match* m, const sind_match_bow* pairs, int B, float nnratio, int check_orientation) {
    sind::BowParams p{}; p.nnratio = nnratio; p.checkOrientation = check_orientation ? 1 : 0;
    return run_bow(m, BowKind{"sind_match_by_bow", "sind_match_by_bow: pair", K_NODE | K_FLAGS | K_ANGLE, K_NODE | K_ANGLE, false, false, sind::launch_match_by_bow}, pairs, B, p);
}

int sind_match_by_bow_kf(sind_match* m, const sind_match_bow_kf* pairs, int B, float nnratio, int check_orientation) {
    sind::BowParams p{}; p.nnratio = nnratio; p.checkOrientation = check_orientation ? 1 : 0;
    const int use = K_NODE | K_FLAGS | K_ANGLE;
    return run_bow(m, BowKind{"sind_match_by_bow_kf", "sind_match_by_bow_kf: pair", use, use, true, false, sind::launch_match_by_bow_kf}, pairs, B, p);
}

int sind_match_for_triangulation(sind_match* m, const sind_match_tri* pairs, int B, int only_stereo, int check_orientation) {
    sind::BowParams p{}; p.onlyStereo = only_stereo ? 1 : 0; p.checkOrientation = check_orientation ? 1 : 0;
    const int useA = K_NODE | K_FLAGS | K_XY | K_ANGLE | K_URIGHT;
    return run_bow(m, BowKind{"sind_match_for_triangulation", "sind_match_for_triangulation: pair", useA, useA | K_OCTAVE, true, true, sind::launch_match_for_triangulation}, pairs, B, p);
}

}  // extern "C"
