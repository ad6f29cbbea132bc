// The matcher handle behind the C ABI "sind_match_*" (include/sind_hip.h) and what more than one family of its entry points uses.  The entry points: capi_match.cpp
// (create, destroy, the projection searches), capi_match_kf.cpp (projections into a key frame), capi_match_bow.cpp (the vocabulary searches), capi_match_ransac.cpp
// (Sim3 and PnP RANSAC), capi_match_opt.cpp (the optimizers), capi_match_map.cpp (map-point upkeep: triangulation, descriptor, normal and depth).  What one family
// alone uses stays in its file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "match.hpp"
#include "host/sim3.hpp"                                              // Sim3Hyp

const int GRID_CELLS = 3072;                                       // Frame's 64 x 48 grid; grid_start has one entry more
const int DESC_WORDS = 8;                                          // a descriptor: 32 bytes from the caller, 8 words for the kernels; staged and counted in words

// A frame's keypoints as the caller passes them, and which of the arrays a search reads besides n and desc.  flags is whatever the search takes for "closed":
// cur_taken (NULL = all free), kf_valid, has_mp1, has_mp2; the kernels read it as zero or not.
enum { K_XY = 1, K_OCTAVE = 2, K_ANGLE = 4, K_URIGHT = 8, K_FLAGS = 16, K_GRID = 32, K_NODE = 64 };
struct Keys { int n; const float* xy; const int* octave; const float* angle; const float* uRight; const uint8_t* desc; const uint8_t* flags; const int* gridStart; const int* gridIdx; const int* node; };

inline void cpy(void* d, const void* s, size_t n) { if (n) std::memcpy(d, s, n); }                          // empty frames may pass NULL arrays
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
inline bool has_null(const Keys& q, int use) {
    return ((use & K_GRID) && !q.gridStart) || (q.n && (!q.desc || ((use & K_XY) && !q.xy) || ((use & K_OCTAVE) && !q.octave) || ((use & K_ANGLE) && !q.angle) || ((use & K_URIGHT) && !q.uRight) ||
                                                        ((use & K_GRID) && !q.gridIdx) || ((use & K_NODE) && !q.node)));
}

// One element of a batch (who: "entry point: pair" or "...: frame"; a: its acting side, q: its searched side), in the order every entry point reports: capacity, then NULL
// arrays (otherNull: one among those that are on neither side), then the contents that can send a kernel out of bounds
inline int check(const char* who, int b, bool otherNull, const Keys& a, int capA, int useA, const Keys& q, int capQ, int useQ) {
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

// The items of a local-BA or essential-graph call, one after the other in a few streams that grow between launches to the largest call seen (host/g2o_lm.hpp: ItemSizes,
// ItemPtrs).  The entry point digests items 0 .. B - 1 into plan, then: reserve, fill and bind every item (host(b), dev(b)), upload, launch, download, wait, store
template <class Plan, class View> struct PackedItems {
    Staged<int> I; Staged<float> Fin, Fout; Staged<double> Din, head; DevBuf<double> D; Staged<View> views; std::vector<Plan> plan;
    std::vector<sind::ItemSizes> at;                               // where item b starts in each stream; at[B]: the totals (intsOutAt and intsOut unused)
    int reserve(int B, size_t maxB) {
        at.assign((size_t)B + 1, sind::ItemSizes{});
        for (int b = 0; b < B; b++) {
            const sind::ItemSizes& z = plan[b].z; const sind::ItemSizes& o = at[b]; sind::ItemSizes& n = at[b + 1];
            n.ints = o.ints + z.ints; n.floatsIn = o.floatsIn + z.floatsIn; n.floatsOut = o.floatsOut + z.floatsOut; n.doublesIn = o.doublesIn + z.doublesIn; n.head = o.head + z.head; n.work = o.work + z.work;
        }
        const sind::ItemSizes& t = at[B];
        SIND_TRY(I.alloc(t.ints + 1)); SIND_TRY(Fin.alloc(t.floatsIn + 1)); SIND_TRY(Fout.alloc(t.floatsOut + 1)); SIND_TRY(Din.alloc(t.doublesIn + 1)); SIND_TRY(head.alloc(t.head + 1));
        SIND_TRY(D.alloc(t.work + 1)); SIND_TRY(views.alloc(maxB));
        for (int b = 0; b < B; b++) cpy(&I.h[at[b].ints], plan[b].I.data(), plan[b].z.ints * sizeof(int));
        return SIND_OK;
    }
    sind::ItemPtrs host(int b) { const sind::ItemSizes& o = at[b]; return {&I.h[o.ints], &Fin.h[o.floatsIn], &Fout.h[o.floatsOut], &Din.h[o.doublesIn], &head.h[o.head], nullptr}; }
    sind::ItemPtrs dev(int b) { const sind::ItemSizes& o = at[b]; return {I.d.p + o.ints, Fin.d.p + o.floatsIn, Fout.d.p + o.floatsOut, Din.d.p + o.doublesIn, head.d.p + o.head, D.p + o.work}; }
    int upload(int B, hipStream_t s) {
        const sind::ItemSizes& t = at[B];
        SIND_TRY(I.up(t.ints, s)); SIND_TRY(Fin.up(t.floatsIn, s)); if (t.doublesIn) SIND_TRY(Din.up(t.doublesIn, s)); SIND_TRY(views.up(B, s));
        return SIND_OK;
    }
    int download(int B, hipStream_t s) {
        for (int b = 0; b < B; b++) {                              // the ints that come back are a range of an item's ints
            const sind::ItemSizes& z = plan[b].z; const size_t o = at[b].ints + z.intsOutAt;
            if (z.intsOut) HIP_TRY(hipMemcpyAsync(&I.h[o], I.d.p + o, z.intsOut * sizeof(int), hipMemcpyDeviceToHost, s));
        }
        SIND_TRY(Fout.down(at[B].floatsOut, s)); SIND_TRY(head.down(at[B].head, s));
        return SIND_OK;
    }
};

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
    // sind_match_local_ba (match_localba.hip) and sind_match_essential_graph (match_essgraph.hip): each its own streams, grown by its own calls
    PackedItems<sind::LbaPlan, sind::LbaView> localba; PackedItems<sind::EssPlan, sind::EssView> ess;
    // sind_match_global_ba (match_globalba.hip): the same streams, the items run one after the other; the scalars of the control flow come back through gbaSc
    PackedItems<sind::GbaPlan, sind::GbaView> globalba; PinnedBuf<double> gbaSc; sind::GbaCounters gbaCount;       // gbaCount: launches and host waits of the last call
    // sind_match_triangulate (match_mappoints.hip): the pairs and the matches of a call, grown to the largest call seen
    struct TriSide { Staged<sind::TriPair> pair; Staged<sind::TriMatch> match; Staged<sind::TriOut> out; std::vector<sind::TriMatch> list; } tri;
    // sind_match_update_points (match_mappoints.hip): the items of a call one after the other, grown to the largest call seen
    struct MapSide {
        Staged<int> obsFirst, obsCount, refObs, obsKf, obsOctave, bestObs; Staged<uint8_t> todo, obsBad, updated; Staged<float> x3Dw, Ow, normal, maxDist, minDist; Staged<uint32_t> obsDesc, descOut;
        int reserve(size_t nKf, size_t nPts, size_t nObs) {
            int r = SIND_OK;
            (r = obsFirst.alloc(nPts)) || (r = obsCount.alloc(nPts)) || (r = refObs.alloc(nPts)) || (r = bestObs.alloc(nPts)) || (r = todo.alloc(nPts)) || (r = updated.alloc(nPts)) ||
                (r = x3Dw.alloc(3 * nPts)) || (r = normal.alloc(3 * nPts)) || (r = maxDist.alloc(nPts)) || (r = minDist.alloc(nPts)) || (r = descOut.alloc(DESC_WORDS * nPts)) ||
                (r = obsKf.alloc(nObs)) || (r = obsOctave.alloc(nObs)) || (r = obsBad.alloc(nObs)) || (r = obsDesc.alloc(DESC_WORDS * nObs)) || (r = Ow.alloc(3 * nKf));
            return r;
        }
    } mapPts;
    int reserve_bow() {
        const size_t B = maxB, nl = B * prm.capLast, nc = B * prm.capCur; int r = SIND_OK;
        (r = last.node.alloc(nl)) || (r = last.xy.alloc(nl * 2)) || (r = last.uRight.alloc(nl)) || (r = cur.node.alloc(nc)) || (r = choice.alloc(nl)) || (r = bow.pose.alloc(B)) ||
            (r = bow.segStart.alloc(nl)) || (r = bow.nSeg.alloc(B)) || (r = bow.nValid.alloc(2 * B)) || (r = bow.sortedA.alloc(nl)) || (r = bow.sortedB.alloc(nc));
        return r;
    }
};

// The tail of every search: the matches ([B][stride]), nmatches and, for the projection searches, rounds come down; then every frame's results go where m->out[b] says
inline int finish(sind_match* m, int B, Staged<int>& matches, size_t stride, bool rounds) {
    hipStream_t s = m->stream;
    SIND_TRY(matches.down(B * stride, s)); SIND_TRY(m->nmatches.down(B, s)); if (rounds) SIND_TRY(m->rounds.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (rounds) m->last_rounds = std::max(0, *std::max_element(m->rounds.h.begin(), m->rounds.h.begin() + B));
    for (int b = 0; b < B; b++) { const sind_match::Result& r = m->out[b]; cpy(r.match, &matches.h[b * stride], (size_t)r.n * sizeof(int)); *r.nmatches = m->nmatches.h[b]; }
    return SIND_OK;
}

// mOw = -Rcw^T * tcw of rows 0..2 of a pose (match_local.hip (2))
inline void camera_centre(const float* T, float* Ow) {
    for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)T[4 * k + r] * (double)T[4 * k + 3]; Ow[r] = (float)(s * -1.0); }
}

// Scw -> rows 0..2 of [Rcw | tcw] (ORBmatcher.cc:298-302, :986-989; match_local.hip (5), (6))
inline void decompose_scw(const float* S, float* T) {
    double d = 0; for (int k = 0; k < 3; k++) d += (double)S[k] * (double)S[k];
    const float scw = (float)std::sqrt(d), inv = (float)(1.0 / (double)scw);
    for (int k = 0; k < 12; k++) T[k] = S[k] * inv;
}

// a key frame's int bounds and the grid cell sizes it copies from its frame (include/KeyFrame.h:185-188; Frame constructors, src/Frame.cc:155-156)
inline void kf_bounds(const float* b, float* kb, float* gridInv) {
    for (int k = 0; k < 4; k++) kb[k] = std::trunc(b[k]);
    gridInv[0] = 64.f / (float)(b[1] - b[0]); gridInv[1] = 48.f / (float)(b[3] - b[2]);
}

inline int check_octaves(const char* who, int b, const Keys& q, int nlevels) {
    for (int i = 0; i < q.n; i++) if (q.octave[i] < 0 || q.octave[i] >= nlevels) { sind_set_error("%s %d: octave %d outside [0,%d)", who, b, q.octave[i], nlevels); return SIND_E_ARG; }
    return SIND_OK;
}

// the opening of the five solver entry points below: the handle, the batch and whether the call's own scalars are in order.  -> SIND_OK, or the error, its text set
inline int solver_prologue(const char* fn, const sind_match* m, const void* items, int B, bool scalars_ok = true) {
    if (!m || B < 0 || (B && !items) || !scalars_ok) { sind_set_error("%s: bad arguments", fn); return SIND_E_ARG; }
    if (B > m->maxB) { sind_set_error("%s: B=%d over max_batch %d", fn, B, m->maxB); return SIND_E_CAPACITY; }
    return SIND_OK;
}
