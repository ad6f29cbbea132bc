// C ABI: projection matcher (include/sind_hip.h, "sind_match_*").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "match.hpp"
#include "host/sim3.hpp"
#include "host/pnp.hpp"
#include "host/pose_opt.hpp"
#include "host/sim3_opt.hpp"
#include "host/local_ba.hpp"
#include "host/essential_graph.hpp"

namespace {
const int GRID_CELLS = 3072;                                       // Frame's 64 x 48 grid; grid_start has one entry more
const int DESC_WORDS = 8;                                          // a descriptor: 32 bytes from the caller, 8 words for the kernels; staged and counted in words

// A frame's keypoints as the caller passes them, and which of the arrays a search reads besides n and desc.  flags is whatever the search takes for "closed":
// cur_taken (NULL = all free), kf_valid, has_mp1, has_mp2; the kernels read it as zero or not.
enum { K_XY = 1, K_OCTAVE = 2, K_ANGLE = 4, K_URIGHT = 8, K_FLAGS = 16, K_GRID = 32, K_NODE = 64 };
struct Keys { int n; const float* xy; const int* octave; const float* angle; const float* uRight; const uint8_t* desc; const uint8_t* flags; const int* gridStart; const int* gridIdx; const int* node; };

void cpy(void* d, const void* s, size_t n) { if (n) std::memcpy(d, s, n); }                          // empty frames may pass NULL arrays
template <class T> void put(Staged<T>& a, size_t at, const void* src, size_t count) { cpy(&a.h[at], src, count * sizeof(T)); }    // at, count: elements of T

// One side of a search, dense [maxB][cap]; stage and upload take the same `use`.  Node ids, and xy and uRight of the acting side, appear with the first vocabulary search.
struct Side {
    int cap = 0;
    Staged<int> n, octave, gridStart, gridIdx, node; Staged<float> xy, angle, uRight; Staged<uint8_t> flags; Staged<uint32_t> desc;
    void stage(int b, const Keys& q, int use) {
        const size_t o = (size_t)b * cap, k = (size_t)q.n;
        n.h[b] = q.n; put(desc, o * DESC_WORDS, q.desc, k * DESC_WORDS);
        if (use & K_XY) put(xy, o * 2, q.xy, k * 2); if (use & K_OCTAVE) put(octave, o, q.octave, k); if (use & K_ANGLE) put(angle, o, q.angle, k); if (use & K_URIGHT) put(uRight, o, q.uRight, k);
        if (use & K_FLAGS) { if (q.flags) put(flags, o, q.flags, k); else std::memset(&flags.h[o], 0, k); }      // never what an earlier call left there
        if (use & K_GRID) { put(gridStart, (size_t)b * (GRID_CELLS + 1), q.gridStart, GRID_CELLS + 1); put(gridIdx, o, q.gridIdx, (size_t)q.gridStart[GRID_CELLS]); }
        if (use & K_NODE) put(node, o, q.node, k);
    }
    int upload(int B, int use, hipStream_t s) {
        const size_t k = (size_t)B * cap;
        SIND_TRY(n.up(B, s)); SIND_TRY(desc.up(k * DESC_WORDS, s));
        if (use & K_XY) SIND_TRY(xy.up(k * 2, s)); if (use & K_OCTAVE) SIND_TRY(octave.up(k, s)); if (use & K_ANGLE) SIND_TRY(angle.up(k, s)); if (use & K_URIGHT) SIND_TRY(uRight.up(k, s));
        if (use & K_FLAGS) SIND_TRY(flags.up(k, s)); if (use & K_NODE) SIND_TRY(node.up(k, s));
        if (use & K_GRID) { SIND_TRY(gridStart.up((size_t)B * (GRID_CELLS + 1), s)); SIND_TRY(gridIdx.up(k, s)); }
        return SIND_OK;
    }
};

// a NULL among the arrays the search reads (flags is for the caller to judge: the projection searches take NULL for "all free")
bool has_null(const Keys& q, int use) {
    return ((use & K_GRID) && !q.gridStart) || (q.n && (!q.desc || ((use & K_XY) && !q.xy) || ((use & K_OCTAVE) && !q.octave) || ((use & K_ANGLE) && !q.angle) || ((use & K_URIGHT) && !q.uRight) ||
                                                        ((use & K_GRID) && !q.gridIdx) || ((use & K_NODE) && !q.node)));
}

// One element of a batch (who: "entry point: pair" or "...: frame"; a: its acting side, q: its searched side), in the order every entry point reports: capacity, then NULL
// arrays (otherNull: one among those that are on neither side), then the contents that can send a kernel out of bounds
int check(const char* who, int b, bool otherNull, const Keys& a, int capA, int useA, const Keys& q, int capQ, int useQ) {
    if (a.n < 0 || a.n > capA || q.n < 0 || q.n > capQ) { sind_set_error("%s %d has %d / %d entries, capacity %d / %d", who, b, a.n, q.n, capA, capQ); return SIND_E_CAPACITY; }
    if (otherNull || has_null(a, useA) || has_null(q, useQ)) { sind_set_error("%s %d: null array", who, b); return SIND_E_ARG; }
    if (useQ & K_GRID) {
        const int* g = q.gridStart; bool ok = g[0] == 0 && g[GRID_CELLS] >= 0 && g[GRID_CELLS] <= q.n;
        for (int c = 0; ok && c < GRID_CELLS; c++) ok = g[c + 1] >= g[c];
        if (!ok) { sind_set_error("%s %d: malformed grid", who, b); return SIND_E_ARG; }
        for (int j = 0; j < g[GRID_CELLS]; j++) if (q.gridIdx[j] < 0 || q.gridIdx[j] >= q.n) { sind_set_error("%s %d: grid index outside the keypoints", who, b); return SIND_E_ARG; }
    }
    if (useQ & K_NODE) for (const Keys* k : {&a, &q}) for (int i = 0; i < k->n; i++) if (k->node[i] < -1) { sind_set_error("%s %d: node id below -1", who, b); return SIND_E_ARG; }
    return SIND_OK;
}
}  // namespace

// The kinds of call share the two sides and the results (last.flags holds valid|has_obs, kf_valid or has_mp1, cur.flags holds cur_taken or has_mp2), so a call stages
// everything it reads.  What only some calls need appears on first use.
struct sind_match {
    int device = 0, maxB = 0; sind::MatchParams prm{}; float mb = 0; hipStream_t stream = nullptr; int last_rounds = 0;
    Side last, cur;                                                // acting side: the last frame's points, side A of the vocabulary searches; searched side: the frame, side B
    Staged<sind::MatchPose> pose; Staged<float> x3Dw;              // of the last frame (sind_match_by_projection)
    Staged<int> matchOfCur, nmatches, rounds;                      // results [maxB][capCur], [maxB], [maxB]
    Staged<int> choice;                                            // [maxB][capLast]: scratch on the device, and match12 of the triangulation, with which its host side appears
    DevBuf<int> minOwner;                                          // scratch [maxB][capCur]
    struct Result { int* match; int n; int* nmatches; };
    std::vector<Result> out;                                       // the caller's outputs of the call in progress, per frame
    DevBuf<float4> curPack;                                        // keypoint records of match_local.hip, on first use
    // map-point side of sind_match_local_map (capacity from sind_match_reserve_map_points) and of sind_match_by_projection_kf (cap_last, on first use)
    struct PointSide {
        int cap = 0;
        Staged<sind::LocalPose> pose; Staged<int> n, level, nToMatch; Staged<float> x3Dw, normal, maxDist, minDist, angle, projXYR, viewCos; Staged<uint8_t> flags, inView; Staged<uint32_t> desc;
        DevBuf<int> choice;
        int reserve(size_t B, int c) {
            const size_t k = B * (size_t)c; int r = SIND_OK;
            if ((r = pose.alloc(B)) || (r = n.alloc(B)) || (r = nToMatch.alloc(B)) || (r = level.alloc(k)) || (r = choice.alloc(k)) || (r = x3Dw.alloc(k * 3)) || (r = normal.alloc(k * 3)) ||
                (r = maxDist.alloc(k)) || (r = minDist.alloc(k)) || (r = angle.alloc(k)) || (r = projXYR.alloc(k * 3)) || (r = viewCos.alloc(k)) || (r = flags.alloc(k)) || (r = inView.alloc(k)) ||
                (r = desc.alloc(k * DESC_WORDS))) return r;
            cap = c; return SIND_OK;
        }
    } local, reloc;
    // sort scratch and pair geometry of sind_match_by_bow / sind_match_for_triangulation (match_bow.hip); with them the two sides get their node ids and side A xy and uRight
    struct BowSide {
        Staged<sind::TriPose> pose; DevBuf<int> segStart, nSeg, nValid; DevBuf<int2> sortedA, sortedB;
    } bow;
    // projections into a key frame (match_fuse.hip), on first use.  fuse: sind_match_fuse, [maxB] items of local.cap points and cap_cur keypoints; sim3: sind_match_by_sim3,
    // [2 maxB] items (pair b, side s -> item 2b + s) of min(cap_last, cap_cur) slots, which are points and keypoints at once
    struct KfSide {
        int capP = 0, capK = 0;
        Staged<sind::KfPose> pose; Staged<int> nP, gridStart, gridIdx, bestIdx, bestDist, count, match12; Staged<float> x3Dw, normal, maxDist, minDist; Staged<uint8_t> valid;
        Staged<uint32_t> ptDesc, keyDesc; Staged<float4> pack;
        int reserve(size_t items, int cp, int ck) {
            const size_t np = items * (size_t)cp, nk = items * (size_t)ck; int r = SIND_OK;
            if ((r = pose.alloc(items)) || (r = nP.alloc(items)) || (r = count.alloc(items)) || (r = gridStart.alloc(items * (GRID_CELLS + 1))) || (r = gridIdx.alloc(nk)) ||
                (r = bestIdx.alloc(np)) || (r = bestDist.alloc(np)) || (r = match12.alloc(np)) || (r = x3Dw.alloc(np * 3)) || (r = normal.alloc(np * 3)) || (r = maxDist.alloc(np)) ||
                (r = minDist.alloc(np)) || (r = valid.alloc(np)) || (r = ptDesc.alloc(np * DESC_WORDS)) || (r = keyDesc.alloc(nk * DESC_WORDS)) || (r = pack.alloc(nk))) return r;
            capP = cp; capK = ck; return SIND_OK;
        }
    } fuse, sim3;
    // sind_match_sim3_ransac (match_sim3.hip), on first use: [maxB] candidates of min(cap_last, cap_cur) correspondences and SIM3_MAX_ITS hypotheses
    struct RansacSide {
        int cap = 0;
        Staged<int> n, nIts, count; Staged<float4> corr; Staged<sind::Sim3Pose> hyp; Staged<unsigned long long> bits; std::vector<sind::Sim3Hyp> solved;
        int reserve(size_t B, int c) {
            const size_t nh = B * SIM3_MAX_ITS; int r = SIND_OK;
            if ((r = n.alloc(B)) || (r = nIts.alloc(B)) || (r = count.alloc(nh)) || (r = corr.alloc(B * 3 * (size_t)c)) || (r = hyp.alloc(nh)) || (r = bits.alloc(nh * (size_t)divup(c, 64)))) return r;
            solved.resize(nh); cap = c; return SIND_OK;
        }
    } ransac;
    // sind_match_pnp_ransac (match_pnp.hip), on first use: [maxB] candidates of min(cap_last, cap_cur) correspondences and PNP_MAX_ITS samples, and one round of Refine problems
    struct PnpSide {
        int cap = 0;
        Staged<int> n, nIts, count, refCount; Staged<float4> pts; Staged<float2> uv; Staged<int4> samples; Staged<unsigned long long> bestBits, bits, refBits;
        Staged<sind::PnpPose> pose, refPose; Staged<sind::PnpRefine> refine; DevBuf<double> work;
        std::vector<int> refineOfHyp, hypOfRefine;
        int reserve(size_t B, int c) {
            const size_t nh = B * PNP_MAX_ITS, w = (size_t)divup(c, 64); int r = SIND_OK;
            if ((r = n.alloc(B)) || (r = nIts.alloc(B)) || (r = count.alloc(nh)) || (r = pts.alloc(B * (size_t)c)) || (r = uv.alloc(B * (size_t)c)) || (r = samples.alloc(nh)) ||
                (r = bestBits.alloc(B * w)) || (r = bits.alloc(nh * w)) || (r = pose.alloc(nh)) || (r = refCount.alloc(PNP_REFINE_SLOTS)) || (r = refBits.alloc(PNP_REFINE_SLOTS * w)) ||
                (r = refPose.alloc(PNP_REFINE_SLOTS)) || (r = refine.alloc(PNP_REFINE_SLOTS)) || (r = work.alloc((size_t)12 * c * PNP_REFINE_SLOTS))) return r;
            refineOfHyp.resize(PNP_MAX_ITS); hypOfRefine.resize(PNP_MAX_ITS + 1); cap = c; return SIND_OK;
        }
    } pnp;
    // sind_match_pose_optimize (match_pose.hip), on first use: [maxB] items of min(cap_last, cap_cur) correspondences
    struct PoseSide {
        int cap = 0;
        Staged<int> n; Staged<float> Tcw; Staged<float4> pts, obs; Staged<uint8_t> outlier; Staged<sind::PoseOptResult> res;
        int reserve(size_t B, int c) {
            int r = SIND_OK;
            if ((r = n.alloc(B)) || (r = Tcw.alloc(B * 16)) || (r = pts.alloc(B * (size_t)c)) || (r = obs.alloc(B * (size_t)c)) || (r = outlier.alloc(B * (size_t)c)) || (r = res.alloc(B))) return r;
            cap = c; return SIND_OK;
        }
    } poseopt;
    // sind_match_sim3_optimize (match_sim3opt.hip), on first use: [maxB] items of min(cap_last, cap_cur) pairs
    struct Sim3OptSide {
        int cap = 0;
        Staged<sind::Sim3OptHead> head; Staged<float4> p1, p2, ob; Staged<uint8_t> removed; Staged<sind::Sim3OptResult> res;
        int reserve(size_t B, int c) {
            int r = SIND_OK;
            if ((r = head.alloc(B)) || (r = p1.alloc(B * (size_t)c)) || (r = p2.alloc(B * (size_t)c)) || (r = ob.alloc(B * (size_t)c)) || (r = removed.alloc(B * (size_t)c)) || (r = res.alloc(B))) return r;
            cap = c; return SIND_OK;
        }
    } sim3opt;
    // sind_match_local_ba (match_localba.hip): the items of a call one after the other in four buffers, grown between calls to the largest call seen
    struct LocalBaSide {
        Staged<int> I; Staged<float> Fin, Fout; DevBuf<double> D; Staged<sind::LbaView> views; Staged<sind::LbaDiag> diag; std::vector<sind::LbaPlan> plan;
    } localba;
    // sind_match_essential_graph (match_essgraph.hip): the same scheme, with the doubles that go up (the Sim3 maps) and those that come down (head)
    struct EssSide {
        Staged<int> I; Staged<float> Fin, Fout; Staged<double> Din, head; DevBuf<double> D; Staged<sind::EssView> views; std::vector<sind::EssPlan> plan;     // head: EssDiag and Siw_out of every item, one after the other
    } ess;
    int reserve_bow() {
        const size_t B = maxB, nl = B * prm.capLast, nc = B * prm.capCur; int r = SIND_OK;
        (r = last.node.alloc(nl)) || (r = last.xy.alloc(nl * 2)) || (r = last.uRight.alloc(nl)) || (r = cur.node.alloc(nc)) || (r = choice.alloc(nl)) || (r = bow.pose.alloc(B)) ||
            (r = bow.segStart.alloc(nl)) || (r = bow.nSeg.alloc(B)) || (r = bow.nValid.alloc(2 * B)) || (r = bow.sortedA.alloc(nl)) || (r = bow.sortedB.alloc(nc));
        return r;
    }
};

namespace {
// The tail of every search: the matches ([B][stride]), nmatches and, for the projection searches, rounds come down; then every frame's results go where m->out[b] says
int finish(sind_match* m, int B, Staged<int>& matches, size_t stride, bool rounds) {
    hipStream_t s = m->stream;
    SIND_TRY(matches.down(B * stride, s)); SIND_TRY(m->nmatches.down(B, s)); if (rounds) SIND_TRY(m->rounds.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (rounds) m->last_rounds = std::max(0, *std::max_element(m->rounds.h.begin(), m->rounds.h.begin() + B));
    for (int b = 0; b < B; b++) { const sind_match::Result& r = m->out[b]; cpy(r.match, &matches.h[b * stride], (size_t)r.n * sizeof(int)); *r.nmatches = m->nmatches.h[b]; }
    return SIND_OK;
}

// CurrentFrame / LastFrame pose algebra of ORBmatcher.cc:1338-1349 (cv::gemm semantics: A*b+c without transposition = FP32 row
// product then FP64 alpha/beta; -A^T*b = FP64 accumulation)
void forward_backward(const float* Tc, const float* Tl, float mb, bool mono, int& fwd, int& bwd) {
    float twc[3], tlc[3];
    for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)Tc[4 * k + r] * (double)Tc[4 * k + 3]; twc[r] = (float)(s * -1.0); }
    for (int r = 0; r < 3; r++) { const float t = Tl[4 * r] * twc[0] + Tl[4 * r + 1] * twc[1] + Tl[4 * r + 2] * twc[2]; tlc[r] = (float)((double)t * 1.0 + (double)Tl[4 * r + 3] * 1.0); }
    fwd = tlc[2] > mb && !mono; bwd = -tlc[2] > mb && !mono;
}

// mOw = -Rcw^T * tcw of rows 0..2 of a pose (match_local.hip (2))
void camera_centre(const float* T, float* Ow) {
    for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)T[4 * k + r] * (double)T[4 * k + 3]; Ow[r] = (float)(s * -1.0); }
}

// Scw -> rows 0..2 of [Rcw | tcw] (ORBmatcher.cc:298-302, :986-989; match_local.hip (5), (6))
void decompose_scw(const float* S, float* T) {
    double d = 0; for (int k = 0; k < 3; k++) d += (double)S[k] * (double)S[k];
    const float scw = (float)std::sqrt(d), inv = (float)(1.0 / (double)scw);
    for (int k = 0; k < 12; k++) T[k] = S[k] * inv;
}

// a key frame's int bounds and the grid cell sizes it copies from its frame (include/KeyFrame.h:185-188; Frame constructors, src/Frame.cc:155-156)
void kf_bounds(const float* b, float* kb, float* gridInv) {
    for (int k = 0; k < 4; k++) kb[k] = std::trunc(b[k]);
    gridInv[0] = 64.f / (float)(b[1] - b[0]); gridInv[1] = 48.f / (float)(b[3] - b[2]);
}

int check_octaves(const char* who, int b, const Keys& q, int nlevels) {
    for (int i = 0; i < q.n; i++) if (q.octave[i] < 0 || q.octave[i] >= nlevels) { sind_set_error("%s %d: octave %d outside [0,%d)", who, b, q.octave[i], nlevels); return SIND_E_ARG; }
    return SIND_OK;
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

// ---- vocabulary-guided searches (match_bow.hip) ----
Keys side_a(const sind_match_bow& q) { return Keys{q.n_kf, nullptr, nullptr, q.kf_angle, nullptr, q.kf_desc, q.kf_valid, nullptr, nullptr, q.kf_node}; }
Keys side_b(const sind_match_bow& q) { return Keys{q.n_cur, nullptr, nullptr, q.cur_angle, nullptr, q.cur_desc, nullptr, nullptr, nullptr, q.cur_node}; }
Keys side_a(const sind_match_bow_kf& q) { return Keys{q.n1, nullptr, nullptr, q.angle1, nullptr, q.desc1, q.valid1, nullptr, nullptr, q.node1}; }
Keys side_b(const sind_match_bow_kf& q) { return Keys{q.n2, nullptr, nullptr, q.angle2, nullptr, q.desc2, q.valid2, nullptr, nullptr, q.node2}; }
Keys side_a(const sind_match_tri& q) { return Keys{q.n1, q.un_xy1, nullptr, q.angle1, q.u_right1, q.desc1, q.has_mp1, nullptr, nullptr, q.node1}; }
Keys side_b(const sind_match_tri& q) { return Keys{q.n2, q.un_xy2, q.octave2, q.angle2, q.u_right2, q.desc2, q.has_mp2, nullptr, nullptr, q.node2}; }

sind::BowParams bow_params(const sind_match* m, int maxN) {
    sind::BowParams p{}; const sind::MatchParams& c = m->prm;
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; std::memcpy(p.scale, c.scale, sizeof(p.scale)); p.capA = c.capLast; p.capB = c.capCur;
    p.sortLen = 1; while (p.sortLen < maxN) p.sortLen <<= 1;
    return p;
}

sind::BowArrays bow_arrays(sind_match* m) {
    Side& l = m->last; Side& c = m->cur; sind_match::BowSide& w = m->bow;
    return sind::BowArrays{l.n.d.p, c.n.d.p, l.node.d.p, c.node.d.p, l.flags.d.p, l.angle.d.p, l.desc.d.p, c.angle.d.p, c.desc.d.p, w.pose.d.p, l.xy.d.p, l.uRight.d.p, c.flags.d.p,
                           c.xy.d.p, c.octave.d.p, c.uRight.d.p, w.sortedA.p, w.sortedB.p, w.segStart.p, w.nSeg.p, w.nValid.p, m->choice.d.p, m->matchOfCur.d.p, m->nmatches.d.p};
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

// the opening of the five solver entry points below: the handle, the batch and whether the call's own scalars are in order.  -> SIND_OK, or the error, its text set
static int solver_prologue(const char* fn, const sind_match* m, const void* items, int B, bool scalars_ok = true) {
    if (!m || B < 0 || (B && !items) || !scalars_ok) { sind_set_error("%s: bad arguments", fn); return SIND_E_ARG; }
    if (B > m->maxB) { sind_set_error("%s: B=%d over max_batch %d", fn, B, m->maxB); return SIND_E_CAPACITY; }
    return SIND_OK;
}

int sind_match_sim3_ransac(sind_match* m, const sind_sim3_item* items, int B, int fix_scale) {
    const char* who = "sind_match_sim3_ransac: item";
    SIND_TRY(solver_prologue("sind_match_sim3_ransac", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int its = 0, maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b];
        if (q.n < 0 || q.n_its < 0) { sind_set_error("%s %d: negative count", who, b); return SIND_E_ARG; }
        if (q.n > cs || q.n_its > SIM3_MAX_ITS) { sind_set_error("%s %d has %d correspondences / %d iterations, capacity %d / %d", who, b, q.n, q.n_its, cs, SIM3_MAX_ITS); return SIND_E_CAPACITY; }
        if ((q.n && (!q.T1w || !q.T2w || !q.x3Dw1 || !q.x3Dw2 || !q.sigma2_1 || !q.sigma2_2)) || (q.n_its && (!q.triple || !q.count || !q.s12 || !q.R12 || !q.t12 || (q.n && !q.inlier_bits)))) {
            sind_set_error("%s %d: null array", who, b); return SIND_E_ARG;
        }
        for (int i = 0; i < q.n; i++) if (!(q.sigma2_1[i] >= 0 && q.sigma2_2[i] >= 0 && std::isfinite(q.sigma2_1[i]) && std::isfinite(q.sigma2_2[i]))) { sind_set_error("%s %d: sigma2 %d is not a finite non-negative number", who, b, i); return SIND_E_ARG; }
        for (int k = 0; k < 3 * q.n_its; k++) if (q.triple[k] < 0 || q.triple[k] >= q.n) { sind_set_error("%s %d: triple index %d outside [0,%d)", who, b, q.triple[k], q.n); return SIND_E_ARG; }
        its = std::max(its, q.n_its); maxN = std::max(maxN, q.n);
    }
    if (!its) return SIND_OK;                                                                          // nothing to evaluate, nothing to write
    HIP_TRY(hipSetDevice(m->device));
    sind_match::RansacSide& w = m->ransac;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::Sim3Params p{c.fx, c.fy, c.cx, c.cy, cs, its, std::max(1, divup(maxN, 64))};
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b];
        float4* c1 = &w.corr.h[(size_t)b * 3 * cs]; float4* c2 = c1 + cs; float4* im = c2 + cs;
        for (int i = 0; i < q.n; i++) {                                                                // the constructor (:84-109)
            float x1[3], x2[3], p1[2], p2[2];
            sind::sim3_to_camera(q.T1w, q.x3Dw1 + 3 * i, x1); sind::sim3_to_camera(q.T2w, q.x3Dw2 + 3 * i, x2);
            sind::sim3_to_image(c.fx, c.fy, c.cx, c.cy, x1, p1); sind::sim3_to_image(c.fx, c.fy, c.cx, c.cy, x2, p2);
            c1[i] = make_float4(x1[0], x1[1], x1[2], sind::sim3_max_error(q.sigma2_1[i])); c2[i] = make_float4(x2[0], x2[1], x2[2], sind::sim3_max_error(q.sigma2_2[i]));
            im[i] = make_float4(p1[0], p1[1], p2[0], p2[1]);
        }
        w.n.h[b] = q.n; w.nIts.h[b] = q.n_its;
        for (int h = 0; h < q.n_its; h++) {                                                            // the sample (:166-177) and ComputeSim3
            float P1[9], P2[9];
            for (int k = 0; k < 3; k++) { const float4 a1 = c1[q.triple[3 * h + k]], a2 = c2[q.triple[3 * h + k]]; P1[k] = a1.x; P1[3 + k] = a1.y; P1[6 + k] = a1.z; P2[k] = a2.x; P2[3 + k] = a2.y; P2[6 + k] = a2.z; }
            sind::Sim3Hyp& s = w.solved[(size_t)b * its + h];
            sind::sim3_horn(P1, P2, fix_scale != 0, s);
            sind::Sim3Pose& d = w.hyp.h[(size_t)b * its + h]; cpy(d.T12, s.T12, sizeof(d.T12)); cpy(d.T21, s.T21, sizeof(d.T21));
        }
    }
    hipStream_t s = m->stream; const size_t nh = (size_t)B * its;
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.nIts.up(B, s)); SIND_TRY(w.corr.up((size_t)B * 3 * cs, s)); SIND_TRY(w.hyp.up(nh, s));
    SIND_TRY(sind::launch_sim3_check(p, sind::Sim3Arrays{w.n.d.p, w.nIts.d.p, w.corr.d.p, w.hyp.d.p, w.count.d.p, w.bits.d.p}, B, s));
    SIND_TRY(w.count.down(nh, s)); SIND_TRY(w.bits.down(nh * p.words, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b]; const int nw = divup(q.n, 64);
        for (int h = 0; h < q.n_its; h++) {
            const size_t o = (size_t)b * its + h; const sind::Sim3Hyp& r = w.solved[o];
            q.count[h] = w.count.h[o]; cpy(q.inlier_bits + (size_t)h * nw, &w.bits.h[o * p.words], (size_t)nw * sizeof(uint64_t));
            q.s12[h] = r.s12; cpy(q.R12 + 9 * h, r.R12, sizeof(r.R12)); cpy(q.t12 + 3 * h, r.t12, sizeof(r.t12));
        }
    }
    return SIND_OK;
}

int sind_match_pnp_ransac(sind_match* m, const sind_pnp_item* items, int B) {
    const char* who = "sind_match_pnp_ransac: item";
    SIND_TRY(solver_prologue("sind_match_pnp_ransac", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int its = 0, maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b];
        if (q.n < 0 || q.n_its < 0 || q.best_count < 0) { sind_set_error("%s %d: negative count", who, b); return SIND_E_ARG; }
        if (q.n > cs || q.n_its > PNP_MAX_ITS) { sind_set_error("%s %d has %d correspondences / %d iterations, capacity %d / %d", who, b, q.n, q.n_its, cs, PNP_MAX_ITS); return SIND_E_CAPACITY; }
        if ((q.n && (!q.x3Dw || !q.p2d || !q.sigma2)) || (q.best_count && !q.best_bits) ||
            (q.n_its && (!q.samples || !q.count || !q.R || !q.t || !q.refine || !q.n_refines || !q.refine_hyp || !q.refine_count || !q.refine_R || !q.refine_t || (q.n && (!q.inlier_bits || !q.refine_bits))))) {
            sind_set_error("%s %d: null array", who, b); return SIND_E_ARG;
        }
        if (q.min_inliers < 1) { sind_set_error("%s %d: min_inliers %d below 1", who, b, q.min_inliers); return SIND_E_ARG; }
        for (int i = 0; i < q.n; i++) if (!(q.sigma2[i] >= 0 && std::isfinite(q.sigma2[i]))) { sind_set_error("%s %d: sigma2 %d is not a finite non-negative number", who, b, i); return SIND_E_ARG; }
        for (int h = 0; h < q.n_its; h++) {
            const int* sm = q.samples + 4 * h;
            for (int k = 0; k < 4; k++) {
                if (sm[k] < 0 || sm[k] >= q.n) { sind_set_error("%s %d: sample index %d outside [0,%d)", who, b, sm[k], q.n); return SIND_E_ARG; }
                for (int j = 0; j < k; j++) if (sm[j] == sm[k]) { sind_set_error("%s %d: sample %d repeats index %d", who, b, h, sm[k]); return SIND_E_ARG; }
            }
        }
        if (q.best_bits) {
            int pc = 0;
            for (int i = 0; i < q.n; i++) pc += (int)((q.best_bits[i >> 6] >> (i & 63)) & 1);
            if (pc != q.best_count) { sind_set_error("%s %d: best_count %d, but best_bits has %d bits set", who, b, q.best_count, pc); return SIND_E_ARG; }
        }
        its = std::max(its, q.n_its); maxN = std::max(maxN, q.n);
    }
    if (!its) return SIND_OK;                                                                          // nothing to evaluate, nothing to write
    HIP_TRY(hipSetDevice(m->device));
    sind_match::PnpSide& w = m->pnp;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::PnpParams p{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, cs, its, std::max(1, divup(maxN, 64))};
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b];
        float4* pt = &w.pts.h[(size_t)b * cs]; float2* uv = &w.uv.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) { pt[i] = make_float4(q.x3Dw[3 * i], q.x3Dw[3 * i + 1], q.x3Dw[3 * i + 2], q.sigma2[i] * q.th2); uv[i] = make_float2(q.p2d[2 * i], q.p2d[2 * i + 1]); }
        w.n.h[b] = q.n; w.nIts.h[b] = q.n_its;
        for (int h = 0; h < q.n_its; h++) w.samples.h[(size_t)b * its + h] = make_int4(q.samples[4 * h], q.samples[4 * h + 1], q.samples[4 * h + 2], q.samples[4 * h + 3]);
        unsigned long long* bb = &w.bestBits.h[(size_t)b * p.words];
        for (int k = 0; k < p.words; k++) bb[k] = (q.best_bits && k < divup(q.n, 64)) ? q.best_bits[k] : 0ull;
    }
    hipStream_t s = m->stream; const size_t nh = (size_t)B * its;
    sind::PnpArrays a{w.n.d.p, w.nIts.d.p, w.pts.d.p, w.uv.d.p, w.samples.d.p, w.bestBits.d.p, w.pose.d.p, w.count.d.p, w.bits.d.p, w.refine.d.p, w.work.p, w.refPose.d.p, w.refCount.d.p, w.refBits.d.p};
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.nIts.up(B, s)); SIND_TRY(w.pts.up((size_t)B * cs, s)); SIND_TRY(w.uv.up((size_t)B * cs, s)); SIND_TRY(w.samples.up(nh, s)); SIND_TRY(w.bestBits.up((size_t)B * p.words, s));
    SIND_TRY(sind::launch_pnp_samples(p, a, B, s));                                                     // 1. pose(4) + check for all hypotheses
    SIND_TRY(w.count.down(nh, s)); SIND_TRY(w.bits.down(nh * p.words, s)); SIND_TRY(w.pose.down(nh, s));
    HIP_TRY(hipStreamSynchronize(s));                                                                   // 2. counts to the host
    struct Slot { int b, r; };
    std::vector<Slot> todo; std::vector<sind::PnpRefine> probs;
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b]; const int nw = divup(q.n, 64);
        if (!q.n_its) { if (q.n_refines) *q.n_refines = 0; continue; }                                 // an item without iterations in a call that has some: no refines
        for (int h = 0; h < q.n_its; h++) {
            const size_t o = (size_t)b * its + h; const sind::PnpPose& r = w.pose.h[o];
            q.count[h] = w.count.h[o]; cpy(q.inlier_bits + (size_t)h * nw, &w.bits.h[o * p.words], (size_t)nw * sizeof(uint64_t));
            cpy(q.R + 9 * h, r.R, sizeof(r.R)); cpy(q.t + 3 * h, r.t, sizeof(r.t));
        }
        const int nr = sind::pnp_refine_plan(q.count, q.n_its, q.min_inliers, q.best_count, q.best_bits != nullptr, w.refineOfHyp.data(), w.hypOfRefine.data());      // 3. the Refine list
        for (int h = 0; h < q.n_its; h++) q.refine[h] = std::max(-1, w.refineOfHyp[h]);              // -2 cannot occur: best_count > 0 comes with best_bits
        *q.n_refines = nr;
        for (int r = 0; r < nr; r++) { q.refine_hyp[r] = w.hypOfRefine[r]; todo.push_back({b, r}); probs.push_back({b, w.hypOfRefine[r]}); }
    }
    for (size_t at = 0; at < todo.size(); at += PNP_REFINE_SLOTS) {                                     // 4. pose(n) + check for the refines, a round of slots at a time
        const int k = (int)std::min<size_t>(PNP_REFINE_SLOTS, todo.size() - at);
        for (int j = 0; j < k; j++) w.refine.h[j] = probs[at + j];
        SIND_TRY(w.refine.up(k, s));
        SIND_TRY(sind::launch_pnp_refines(p, a, k, s));
        SIND_TRY(w.refCount.down(k, s)); SIND_TRY(w.refBits.down((size_t)k * p.words, s)); SIND_TRY(w.refPose.down(k, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int j = 0; j < k; j++) {                                                                  // 5. results back
            const sind_pnp_item& q = items[todo[at + j].b]; const int r = todo[at + j].r, nw = divup(q.n, 64); const sind::PnpPose& o = w.refPose.h[j];
            q.refine_count[r] = w.refCount.h[j]; cpy(q.refine_bits + (size_t)r * nw, &w.refBits.h[(size_t)j * p.words], (size_t)nw * sizeof(uint64_t));
            cpy(q.refine_R + 9 * r, o.R, sizeof(o.R)); cpy(q.refine_t + 3 * r, o.t, sizeof(o.t));
        }
    }
    return SIND_OK;
}

int sind_match_pose_optimize(sind_match* m, const sind_poseopt_item* items, int B) {
    const char* who = "sind_match_pose_optimize: item";
    SIND_TRY(solver_prologue("sind_match_pose_optimize", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_poseopt_item& q = items[b];
        if (q.n > cs) { sind_set_error("%s %d has %d correspondences, capacity %d", who, b, q.n, cs); return SIND_E_CAPACITY; }
        static const char* const what[] = {"", "negative count", "null array", "an inv_sigma2 is not a finite non-negative number", "the pose is not finite"};
        if (const int bad = sind::poseopt_check(q)) { sind_set_error("%s %d: %s", who, b, what[bad]); return SIND_E_ARG; }
        maxN = std::max(maxN, q.n);
    }
    if (!B) return SIND_OK;
    static_assert(sizeof(sind::PoseOptResult) == sizeof(sind::PoseOptOut), "PoseOptResult is PoseOptOut");
    if (maxN < 3) {                                                                                     // the reference's `return 0` for every item: nothing to launch
        for (int b = 0; b < B; b++) { *items[b].n_good = 0; *items[b].n_rounds = 0; }
        return SIND_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    sind_match::PoseSide& w = m->poseopt;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::PoseOptParams p{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf, cs};
    for (int b = 0; b < B; b++) {
        const sind_poseopt_item& q = items[b];
        float4* pt = &w.pts.h[(size_t)b * cs]; float4* ob = &w.obs.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) { pt[i] = make_float4(q.x3Dw[3 * i], q.x3Dw[3 * i + 1], q.x3Dw[3 * i + 2], q.inv_sigma2[i]); ob[i] = make_float4(q.obs_xy[2 * i], q.obs_xy[2 * i + 1], q.u_right[i], 0.f); }
        w.n.h[b] = q.n; cpy(&w.Tcw.h[(size_t)b * 16], q.Tcw, 16 * sizeof(float));
    }
    hipStream_t s = m->stream; const size_t k = (size_t)B * cs;
    sind::PoseOptArrays a{w.n.d.p, w.Tcw.d.p, w.pts.d.p, w.obs.d.p, w.outlier.d.p, w.res.d.p};
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.Tcw.up((size_t)B * 16, s)); SIND_TRY(w.pts.up(k, s)); SIND_TRY(w.obs.up(k, s));
    SIND_TRY(sind::launch_pose_optimize(p, a, B, s));
    SIND_TRY(w.outlier.down(k, s)); SIND_TRY(w.res.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        sind::PoseOptOut o; std::memcpy(&o, &w.res.h[b], sizeof(o));
        sind::poseopt_store(items[b], o, &w.outlier.h[(size_t)b * cs]);
    }
    return SIND_OK;
}

int sind_match_sim3_optimize(sind_match* m, const sind_sim3opt_item* items, int B, float th2, int fix_scale) {
    const char* who = "sind_match_sim3_optimize: item";
    SIND_TRY(solver_prologue("sind_match_sim3_optimize", m, items, B, std::isfinite(th2) && th2 >= 0));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_sim3opt_item& q = items[b];
        if (q.n > cs) { sind_set_error("%s %d has %d pairs, capacity %d", who, b, q.n, cs); return SIND_E_CAPACITY; }
        static const char* const what[] = {"", "negative count", "null array", "an inv_sigma2 is not a finite non-negative number", "the input Sim3 or an intrinsic is not finite"};
        if (const int bad = sind::sim3opt_check(q)) { sind_set_error("%s %d: %s", who, b, what[bad]); return SIND_E_ARG; }
        maxN = std::max(maxN, q.n);
    }
    if (!B) return SIND_OK;
    static_assert(sizeof(sind::Sim3OptResult) == sizeof(sind::Sim3OptOut), "Sim3OptResult is Sim3OptOut");
    if (maxN < 1) {                                                                                     // every graph is empty: the reference's `return 0`, nothing to launch
        for (int b = 0; b < B; b++) {
            sind::Sim3Q S0; sind::s3_from_input(items[b].s12, items[b].R12, items[b].t12, S0);
            sind::Sim3OptOut o{}; std::memcpy(o.q, S0.q, sizeof(o.q)); std::memcpy(o.t, S0.t, sizeof(o.t)); o.s = S0.s;
            sind::sim3opt_store(items[b], o, nullptr);
        }
        return SIND_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    sind_match::Sim3OptSide& w = m->sim3opt;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::Sim3OptParams p{th2, fix_scale != 0, cs};
    for (int b = 0; b < B; b++) {
        const sind_sim3opt_item& q = items[b];
        float4* p1 = &w.p1.h[(size_t)b * cs]; float4* p2 = &w.p2.h[(size_t)b * cs]; float4* ob = &w.ob.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) {
            p1[i] = make_float4(q.x3Dc1[3 * i], q.x3Dc1[3 * i + 1], q.x3Dc1[3 * i + 2], q.inv_sigma2_1[i]);
            p2[i] = make_float4(q.x3Dc2[3 * i], q.x3Dc2[3 * i + 1], q.x3Dc2[3 * i + 2], q.inv_sigma2_2[i]);
            ob[i] = make_float4(q.obs1_xy[2 * i], q.obs1_xy[2 * i + 1], q.obs2_xy[2 * i], q.obs2_xy[2 * i + 1]);
        }
        sind::Sim3OptHead& h = w.head.h[b];
        cpy(h.K1, q.K1, 4 * sizeof(float)); cpy(h.K2, q.K2, 4 * sizeof(float)); h.s12 = q.s12; cpy(h.R12, q.R12, 9 * sizeof(float)); cpy(h.t12, q.t12, 3 * sizeof(float)); h.n = q.n;
    }
    hipStream_t s = m->stream; const size_t k = (size_t)B * cs;
    sind::Sim3OptArrays a{w.head.d.p, w.p1.d.p, w.p2.d.p, w.ob.d.p, w.removed.d.p, w.res.d.p};
    SIND_TRY(w.head.up(B, s)); SIND_TRY(w.p1.up(k, s)); SIND_TRY(w.p2.up(k, s)); SIND_TRY(w.ob.up(k, s));
    SIND_TRY(sind::launch_sim3_optimize(p, a, B, s));
    SIND_TRY(w.removed.down(k, s)); SIND_TRY(w.res.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        sind::Sim3OptOut o; std::memcpy(&o, &w.res.h[b], sizeof(o));
        sind::sim3opt_store(items[b], o, &w.removed.h[(size_t)b * cs]);
    }
    return SIND_OK;
}

int sind_match_local_ba(sind_match* m, const sind_localba_item* items, int B) {
    const char* who = "sind_match_local_ba: item";
    SIND_TRY(solver_prologue("sind_match_local_ba", m, items, B));
    for (int b = 0; b < B; b++) if (const int bad = sind::lba_check(items[b])) { sind_set_error("%s %d: %s", who, b, sind::lba_check_text[bad]); return SIND_E_ARG; }
    if (!B) return SIND_OK;
    sind_match::LocalBaSide& w = m->localba;
    w.plan.resize((size_t)m->maxB);
    std::vector<size_t> oI((size_t)B + 1, 0), oFi((size_t)B + 1, 0), oFo((size_t)B + 1, 0), oD((size_t)B + 1, 0);
    for (int b = 0; b < B; b++) {
        sind::LbaPlan& pl = w.plan[b];
        if (sind::lba_plan(items[b], pl)) {
            sind_set_error("%s %d is beyond a limit: %d key frames of kind 0, %d key frames, %d points, %d observations, %d co-observation entries", who, b, LBA_MAX_POSES, LBA_MAX_KF, LBA_MAX_MP, LBA_MAX_OBS, LBA_MAX_PAIRS);
            return SIND_E_CAPACITY;
        }
        oI[b + 1] = oI[b] + pl.nI; oFi[b + 1] = oFi[b] + sind::lba_floats_in(pl); oFo[b + 1] = oFo[b] + sind::lba_floats_out(pl); oD[b + 1] = oD[b] + pl.nD;
    }
    HIP_TRY(hipSetDevice(m->device));
    SIND_TRY(w.I.alloc(oI[B] + 1)); SIND_TRY(w.Fin.alloc(oFi[B] + 1)); SIND_TRY(w.Fout.alloc(oFo[B] + 1)); SIND_TRY(w.D.alloc(oD[B] + 1));       // grown here, between launches
    SIND_TRY(w.views.alloc((size_t)m->maxB)); SIND_TRY(w.diag.alloc((size_t)m->maxB));
    const sind::MatchParams& c = m->prm;
    const sind::PoseOptCam K{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf};
    for (int b = 0; b < B; b++) {
        const sind::LbaPlan& pl = w.plan[b];
        cpy(&w.I.h[oI[b]], pl.I.data(), pl.nI * sizeof(int));
        sind::lba_fill_floats(items[b], &w.Fin.h[oFi[b]]);
        sind::lba_bind(pl, items[b].do_more, K, w.I.d.p + oI[b], w.Fin.d.p + oFi[b], w.Fout.d.p + oFo[b], w.D.p + oD[b], w.views.h[b]);
        w.views.h[b].diag = w.diag.d.p + b;
    }
    hipStream_t s = m->stream;
    SIND_TRY(w.I.up(oI[B], s)); SIND_TRY(w.Fin.up(oFi[B], s)); SIND_TRY(w.views.up(B, s));
    SIND_TRY(sind::launch_local_ba(w.views.d.p, B, s));
    for (int b = 0; b < B; b++) {                                                                       // the erase flags are the tail of an item's ints
        const sind::LbaPlan& pl = w.plan[b];
        if (pl.nObs) HIP_TRY(hipMemcpyAsync(&w.I.h[oI[b] + pl.oErase], w.I.d.p + oI[b] + pl.oErase, (size_t)pl.nObs * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    SIND_TRY(w.Fout.down(oFo[B], s)); SIND_TRY(w.diag.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) sind::lba_store(items[b], w.plan[b], &w.I.h[oI[b] + w.plan[b].oErase], &w.Fout.h[oFo[b]], w.diag.h[b]);
    return SIND_OK;
}

int sind_match_essential_graph(sind_match* m, const sind_essgraph_item* items, int B, int fix_scale) {
    const char* who = "sind_match_essential_graph: item";
    SIND_TRY(solver_prologue("sind_match_essential_graph", m, items, B));
    for (int b = 0; b < B; b++) if (const int bad = sind::ess_check(items[b])) { sind_set_error("%s %d: %s", who, b, sind::ess_check_text[bad]); return SIND_E_ARG; }
    if (!B) return SIND_OK;
    sind_match::EssSide& w = m->ess;
    w.plan.resize((size_t)m->maxB);
    std::vector<size_t> oI((size_t)B + 1, 0), oFi((size_t)B + 1, 0), oFo((size_t)B + 1, 0), oDi((size_t)B + 1, 0), oDo((size_t)B + 1, 0), oD((size_t)B + 1, 0);
    int maxMp = 0;
    for (int b = 0; b < B; b++) {
        sind::EssPlan& pl = w.plan[b];
        if (sind::ess_plan(items[b], pl)) {
            sind_set_error("%s %d is beyond a limit: %d key frames, %d edges, %d points, %d entries of the factor's envelope", who, b, ESS_MAX_KF, ESS_MAX_EDGES, ESS_MAX_MP, ESS_MAX_ENV);
            return SIND_E_CAPACITY;
        }
        oI[b + 1] = oI[b] + pl.nI; oFi[b + 1] = oFi[b] + sind::ess_floats_in(pl); oFo[b + 1] = oFo[b] + sind::ess_floats_out(pl); oDi[b + 1] = oDi[b] + sind::ess_doubles_in(pl);
        oDo[b + 1] = oDo[b] + sind::ess_doubles_out(pl); oD[b + 1] = oD[b] + pl.nD;
        maxMp = std::max(maxMp, pl.nMp);
    }
    HIP_TRY(hipSetDevice(m->device));
    SIND_TRY(w.I.alloc(oI[B] + 1)); SIND_TRY(w.Fin.alloc(oFi[B] + 1)); SIND_TRY(w.Fout.alloc(oFo[B] + 1)); SIND_TRY(w.Din.alloc(oDi[B] + 1)); SIND_TRY(w.D.alloc(oD[B] + 1));   // grown here, between launches
    SIND_TRY(w.views.alloc((size_t)m->maxB));
    SIND_TRY(w.head.alloc(oDo[B] + 1));
    for (int b = 0; b < B; b++) {
        const sind::EssPlan& pl = w.plan[b];
        cpy(&w.I.h[oI[b]], pl.I.data(), pl.nI * sizeof(int));
        sind::ess_fill(items[b], &w.Fin.h[oFi[b]], &w.Din.h[oDi[b]]);
        sind::ess_bind(pl, fix_scale, w.I.d.p + oI[b], w.Fin.d.p + oFi[b], w.Din.d.p + oDi[b], w.Fout.d.p + oFo[b], w.D.p + oD[b], w.views.h[b]);
        w.views.h[b].diag = (sind::EssDiag*)(w.head.d.p + oDo[b]); w.views.h[b].SiwOut = w.head.d.p + oDo[b] + 8;                           // what comes down lies together
    }
    hipStream_t s = m->stream;
    SIND_TRY(w.I.up(oI[B], s)); SIND_TRY(w.Fin.up(oFi[B], s)); SIND_TRY(w.Din.up(oDi[B], s)); SIND_TRY(w.views.up(B, s));
    SIND_TRY(sind::launch_essential_graph(w.views.d.p, B, maxMp, s));
    SIND_TRY(w.head.down(oDo[B], s));
    SIND_TRY(w.Fout.down(oFo[B], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) sind::ess_store(items[b], w.plan[b], &w.Fout.h[oFo[b]], &w.head.h[oDo[b]]);
    return SIND_OK;
}

int sind_match_by_bow(sind_match* m, const sind_match_bow* pairs, int B, float nnratio, int check_orientation) {
    const char* who = "sind_match_by_bow: pair";
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("sind_match_by_bow: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int useA = K_NODE | K_FLAGS | K_ANGLE, useB = K_NODE | K_ANGLE, cl = std::min(m->last.cap, BOW_MAX_KEYS), cc = std::min(m->cur.cap, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const sind_match_bow& q = pairs[b];
        SIND_TRY(check(who, b, !q.nmatches || (q.n_cur && !q.match_of_cur) || (q.n_kf && !q.kf_valid), side_a(q), cl, useA, side_b(q), cc, useB));
        maxN = std::max(maxN, std::max(q.n_kf, q.n_cur));
    }
    SIND_TRY(m->reserve_bow());
    for (int b = 0; b < B; b++) { const sind_match_bow& q = pairs[b]; m->last.stage(b, side_a(q), useA); m->cur.stage(b, side_b(q), useB); m->out[b] = {q.match_of_cur, q.n_cur, q.nmatches}; }
    hipStream_t s = m->stream;
    SIND_TRY(m->last.upload(B, useA, s)); SIND_TRY(m->cur.upload(B, useB, s));
    sind::BowParams p = bow_params(m, maxN); p.nnratio = nnratio; p.checkOrientation = check_orientation ? 1 : 0;
    SIND_TRY(sind::launch_match_by_bow(p, bow_arrays(m), B, s));
    return finish(m, B, m->matchOfCur, m->cur.cap, false);
}

int sind_match_by_bow_kf(sind_match* m, const sind_match_bow_kf* pairs, int B, float nnratio, int check_orientation) {
    const char* who = "sind_match_by_bow_kf: pair";
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("sind_match_by_bow_kf: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int use = K_NODE | K_FLAGS | K_ANGLE, cl = std::min(m->last.cap, BOW_MAX_KEYS), cc = std::min(m->cur.cap, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const sind_match_bow_kf& q = pairs[b];
        SIND_TRY(check(who, b, !q.nmatches || (q.n1 && (!q.match12 || !q.valid1)) || (q.n2 && !q.valid2), side_a(q), cl, use, side_b(q), cc, use));
        maxN = std::max(maxN, std::max(q.n1, q.n2));
    }
    SIND_TRY(m->reserve_bow());
    for (int b = 0; b < B; b++) { const sind_match_bow_kf& q = pairs[b]; m->last.stage(b, side_a(q), use); m->cur.stage(b, side_b(q), use); m->out[b] = {q.match12, q.n1, q.nmatches}; }
    hipStream_t s = m->stream;
    SIND_TRY(m->last.upload(B, use, s)); SIND_TRY(m->cur.upload(B, use, s));
    sind::BowParams p = bow_params(m, maxN); p.nnratio = nnratio; p.checkOrientation = check_orientation ? 1 : 0;
    SIND_TRY(sind::launch_match_by_bow_kf(p, bow_arrays(m), B, s));
    return finish(m, B, m->choice, m->last.cap, false);
}

int sind_match_for_triangulation(sind_match* m, const sind_match_tri* pairs, int B, int only_stereo, int check_orientation) {
    const char* who = "sind_match_for_triangulation: pair";
    if (!m || !pairs || B < 1 || B > m->maxB) { sind_set_error("sind_match_for_triangulation: bad arguments (B=%d, max %d)", B, m ? m->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    const int useA = K_NODE | K_FLAGS | K_XY | K_ANGLE | K_URIGHT, useB = useA | K_OCTAVE, cl = std::min(m->last.cap, BOW_MAX_KEYS), cc = std::min(m->cur.cap, BOW_MAX_KEYS);
    int maxN = 1;
    for (int b = 0; b < B; b++) {
        const sind_match_tri& q = pairs[b];
        SIND_TRY(check(who, b, !q.Tcw2 || !q.Cw1 || !q.F12 || !q.nmatches || (q.n1 && (!q.match12 || !q.has_mp1)) || (q.n2 && !q.has_mp2), side_a(q), cl, useA, side_b(q), cc, useB));
        for (int i = 0; i < q.n2; i++) if (q.octave2[i] < 0 || q.octave2[i] >= m->prm.nlevels) { sind_set_error("%s %d: octave %d outside [0,%d)", who, b, q.octave2[i], m->prm.nlevels); return SIND_E_ARG; }
        maxN = std::max(maxN, std::max(q.n1, q.n2));
    }
    SIND_TRY(m->reserve_bow());
    sind_match::BowSide& w = m->bow;
    for (int b = 0; b < B; b++) {
        const sind_match_tri& q = pairs[b];
        sind::TriPose& ps = w.pose.h[b]; cpy(ps.Tcw2, q.Tcw2, sizeof(ps.Tcw2)); cpy(ps.Cw1, q.Cw1, sizeof(ps.Cw1)); cpy(ps.F12, q.F12, sizeof(ps.F12));
        m->last.stage(b, side_a(q), useA); m->cur.stage(b, side_b(q), useB); m->out[b] = {q.match12, q.n1, q.nmatches};
    }
    hipStream_t s = m->stream;
    SIND_TRY(w.pose.up(B, s)); SIND_TRY(m->last.upload(B, useA, s)); SIND_TRY(m->cur.upload(B, useB, s));
    sind::BowParams p = bow_params(m, maxN); p.onlyStereo = only_stereo ? 1 : 0; p.checkOrientation = check_orientation ? 1 : 0;
    SIND_TRY(sind::launch_match_for_triangulation(p, bow_arrays(m), B, s));
    return finish(m, B, m->choice, m->last.cap, false);
}

}  // extern "C"
