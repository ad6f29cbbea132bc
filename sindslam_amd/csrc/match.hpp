// Matcher interface: projection searches (reference src/ORBmatcher.cc:45-129, :1328-1470, :1472-1599; kernels in match_kernels.hip, match_local.hip),
// vocabulary-guided searches (:159-288, :657-823; match_bow.hip, bow_kernels.hip) and projections into a key frame (:290-403, :825-1326; match_fuse.hip).
#pragma once
#include "common.hpp"
#include "host/local_ba.hpp"
#include "host/essential_graph.hpp"
#include "host/global_ba.hpp"
#include "host/map_points.hpp"

namespace sind {

struct MatchParams {
    float fx, fy, cx, cy, bf, bounds[4], th; float scale[16]; int nlevels;
    int capLast, capCur, checkOrientation;
};
struct MatchPose { float Tcw[12]; int forward, backward; };       // per pair: rows 0..2 of CurrentFrame.mTcw, bForward / bBackward

struct MatchArrays {                                              // device pointers, dense [B][cap...]
    const MatchPose* pose; const int* nLast; const int* nCur;
    const float* x3Dw; const uint8_t* lastFlags /* bit0 valid, bit1 has observations */; const int* lastOctave; const float* lastAngle; const uint32_t* lastDesc;
    const float* curUnXY; const int* curOctave; const float* curAngle; const float* curURight; const uint32_t* curDesc; const int* gridStart; const int* gridIdx;
    const uint8_t* curTaken;
    int* choice; int* minOwner;                                   // scratch [B][capLast], [B][capCur]
    int* matchOfCur; int* nmatches; int* rounds;                  // outputs [B][capCur], [B], [B]
};

int launch_search_by_projection(const MatchParams& p, const MatchArrays& a, int B, hipStream_t s);

// Local-map search and relocalisation search (match_local.hip): the points are map points (or a key frame's slots), not a last frame's keypoints.
struct LocalParams {
    float fx, fy, cx, cy, bf, bounds[4], th, nnratio, viewCosLimit, logScaleFactor; float scale[16]; int nlevels;
    int capPts, capCur, orbDist, checkOrientation;
    float gridInv[2];                                             // mode 2 only: a key frame's mfGridElementWidthInv / HeightInv, which are not those of its (int) bounds
};
struct LocalPose { float Tcw[12]; float Ow[3]; };                // per frame: rows 0..2 of CurrentFrame.mTcw, camera centre mOw

struct LocalArrays {                                              // device pointers, dense [B][cap...]
    const LocalPose* pose; const int* nPts; const int* nCur;
    const float* x3Dw; const float* normal; const float* maxDist; const float* minDist; const uint8_t* flags /* bit0 candidate, bit1 closes its keypoint */;
    const float* ptAngle; const uint32_t* ptDesc;
    const float* curUnXY; const int* curOctave; const float* curAngle; const float* curURight; const uint32_t* curDesc; const int* gridStart; const int* gridIdx;
    const uint8_t* curTaken;
    uint8_t* inView; float* projXYR; int* level; float* viewCos; int* nToMatch;      // frustum outputs [B][capPts] (projXYR x3), [B]
    int* choice; int* minOwner; float4* curPack;                  // scratch [B][capPts], [B][capCur], [B][capCur]
    int* matchOfCur; int* nmatches; int* rounds;                  // outputs [B][capCur], [B], [B]
};

// mode 0: Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th); mode 1: SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist);
// mode 2 (search only, after launch_project_kf): SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
int launch_project_points(const LocalParams& p, const LocalArrays& a, int B, int reloc, hipStream_t s);
int launch_search_points(const LocalParams& p, const LocalArrays& a, int B, int mode, hipStream_t s);

// Projections of map points into a key frame (match_fuse.hip).  KF_FUSE, KF_FUSE_SIM3 and KF_BY_SIM3 have no dependence between points: one launch over
// (blocks of points) x items; KF_BY_SIM3 runs 2B items (item 2b + s = the slots of side s of pair b, searched against the keys of item 2b + 1 - s) and then the
// agreement pass.  KF_PROJ_SIM3 projects into LocalArrays (launch_project_kf) and resolves its closed keypoints in launch_search_points(mode 2).
enum { KF_FUSE = 0, KF_FUSE_SIM3 = 1, KF_PROJ_SIM3 = 2, KF_BY_SIM3 = 3 };
struct KfParams {
    float fx, fy, cx, cy, bf, bounds[4] /* the key frame's: int */, gridInv[2], th, logScaleFactor; float scale[16], invSigma2[16]; int nlevels;
    int capPts, capKeys, thDist /* TH_LOW or TH_HIGH */;
};
struct KfPose { float T[12]; float Ow[3]; float T2[12]; };         // per item: rows 0..2 of [Rcw | tcw], camera centre; KF_BY_SIM3: T = the side's own pose, T2 = [sR21 | t21] or [sR12 | t12]
struct KfArrays {                                                 // device pointers, dense [items][cap...]
    const KfPose* pose; const int* nPts;
    const float* x3Dw; const float* normal; const float* maxDist; const float* minDist; const uint8_t* valid; const uint32_t* ptDesc;
    const float4* keyPack /* x, y, uRight, octave */; const uint32_t* keyDesc; const int* gridStart; const int* gridIdx;
    int* bestIdx; int* bestDist; int* count;                      // outputs [items][capPts] x2, [items] (zeroed by the caller; KF_BY_SIM3: [B], written by the agreement pass)
    int* match12;                                                 // KF_BY_SIM3: output [B][capPts]
};
int launch_search_kf(const KfParams& p, const KfArrays& a, int items, int mode, hipStream_t s);
int launch_sim3_agree(const KfParams& p, const KfArrays& a, int B, hipStream_t s);
int launch_project_kf(const LocalParams& p, const LocalArrays& a, int B, hipStream_t s);

// Sim3Solver::CheckInliers for every (candidate, hypothesis) of a call (match_sim3.hip).  The hypotheses come from the host (host/sim3.cpp).
#define SIM3_MAX_ITS 300                                          // mRansacMaxIts of LoopClosing::ComputeSim3
struct Sim3Params { float fx, fy, cx, cy; int cap /* correspondences per candidate */, its /* hypotheses per candidate, this call */, words /* >= ceil(n / 64) of every candidate */; };
struct Sim3Pose { float T12[12], T21[12]; };                       // rows 0..2 of mT12i, mT21i
struct Sim3Arrays {                                               // device pointers
    const int* n; const int* nIts;                                // [B]
    const float4* corr;                                           // [B][3][cap]: (mvX3Dc1, mvnMaxError1), (mvX3Dc2, mvnMaxError2), (mvP1im1, mvP2im2)
    const Sim3Pose* hyp;                                          // [B][its]
    int* count; unsigned long long* bits;                         // outputs [B][its], [B][its][words]: mnInliersi, mvbInliersi (bit i & 63 of word i >> 6)
};
int launch_sim3_check(const Sim3Params& p, const Sim3Arrays& a, int B, hipStream_t s);

// PnPsolver: EPnP and CheckInliers for every (candidate, sample) of a call, and for the Refine problems that follow from their counts (match_pnp.hip, host/epnp.hpp)
#define PNP_MAX_ITS 300                                           // mRansacMaxIts of Tracking::Relocalization
#define PNP_REFINE_SLOTS 32                                       // Refine problems per round: each holds 12 cap doubles of workspace
struct PnpParams { double fu, fv, uc, vc; int cap /* correspondences per candidate */, its /* samples per candidate, this call */, words /* >= ceil(n / 64) of every candidate */; };
struct PnpPose { double R[9], t[3]; };                            // mRi (row-major), mti
struct PnpRefine { int b, hyp; };                                 // candidate; the iteration whose inlier bits are the set, -1: the candidate's bestBits
struct PnpArrays {                                                // device pointers
    const int* n; const int* nIts;                                // [B]
    const float4* pts; const float2* uv;                          // [B][cap]: (mvP3Dw, mvMaxError), mvP2D
    const int4* samples;                                          // [B][its]
    const unsigned long long* bestBits;                           // [B][words]
    PnpPose* pose; int* count; unsigned long long* bits;          // outputs [B][its], [B][its], [B][its][words]
    const PnpRefine* refine;                                      // [PNP_REFINE_SLOTS], this round's
    double* work;                                                 // [12 cap][PNP_REFINE_SLOTS]: pws, us, alphas, pcs of every slot, slots interleaved
    PnpPose* refPose; int* refCount; unsigned long long* refBits; // outputs [PNP_REFINE_SLOTS], .., [PNP_REFINE_SLOTS][words]
};
int launch_pnp_samples(const PnpParams& p, const PnpArrays& a, int B, hipStream_t s);        // compute_pose + CheckInliers of every sample
int launch_pnp_refines(const PnpParams& p, const PnpArrays& a, int nRefines, hipStream_t s); // Refine(): compute_pose on an inlier set + CheckInliers

// Optimizer::PoseOptimization, whole, one workgroup per item (match_pose.hip, host/pose_opt.hpp)
struct PoseOptParams { double fx, fy, cx, cy, bf; int cap /* correspondences per item */; };
struct PoseOptResult { float Tcw[16]; int nGood, nRounds, iters[4], nbad[4]; double pose[4][12], chi2[4], lambda[4]; };    // = sind::PoseOptOut of pose_opt.hpp
struct PoseOptArrays {                                            // device pointers
    const int* n; const float* Tcw;                               // [B], [B][16]
    const float4* pts; const float4* obs;                         // [B][cap]: (Xw, invSigma2), (kpUn.pt, mvuRight, unused)
    uint8_t* outlier; PoseOptResult* res;                         // outputs [B][cap] (mvbOutlier = the edge's level, the kernel's working state too), [B]
};
int launch_pose_optimize(const PoseOptParams& p, const PoseOptArrays& a, int B, hipStream_t s);

// Optimizer::OptimizeSim3, whole, one workgroup per item (match_sim3opt.hip, host/sim3_opt.hpp)
struct Sim3OptParams { float th2; int fixScale; int cap /* pairs per item */; };
struct Sim3OptHead { float K1[4], K2[4], s12, R12[9], t12[3]; int n; };               // per item: fx fy cx cy of both key frames, the input Sim3, the pair count
struct Sim3OptResult { double q[4], t[3], s; int nIn, nBad, stages, iters[2]; double chi2[2], lambda[2]; };              // = sind::Sim3OptOut of sim3_opt.hpp
struct Sim3OptArrays {                                            // device pointers
    const Sim3OptHead* head;                                      // [B]
    const float4* p1; const float4* p2; const float4* ob;         // [B][cap]: (X1c, invSigma2_1), (X2c, invSigma2_2), (obs1, obs2)
    uint8_t* removed; Sim3OptResult* res;                         // outputs [B][cap] (the kernel's working state too), [B]
};
int launch_sim3_optimize(const Sim3OptParams& p, const Sim3OptArrays& a, int B, hipStream_t s);

// Optimizer::LocalBundleAdjustment, whole, one workgroup per item (match_localba.hip, host/local_ba.hpp).  views [B]: device pointers throughout
#define LBA_THREADS 512                                              // profiles/match_local_ba.txt: the compiler's resource report and the choice
int launch_local_ba(const LbaView* views, int B, hipStream_t s);

// Optimizer::OptimizeEssentialGraph, whole: k_ess_graph, one workgroup per item, then k_ess_points over the points of all items on the same stream (match_essgraph.hip,
// host/essential_graph.hpp).  views [B]: device pointers throughout; maxMp: the largest n_mp of the call
#define ESS_THREADS 512                                              // profiles/match_essential_graph.txt: the compiler's resource report and the choice
#define ESS_PT_THREADS 256
#define ESS_PT_BLOCKS 64                                             // per item: a full grid covers 16384 points in one pass, the lanes stride beyond it
int launch_essential_graph(const EssView* views, int B, int maxMp, hipStream_t s);

// Optimizer::BundleAdjustment, the optimize of a global BA: kernels per phase over the whole grid on stream s, the Levenberg-Marquardt driver on the host
// (match_globalba.hip, host/global_ba.hpp).  w: device pointers throughout; cs: GbaPlan::cs; pinned: [BA_SC_N] page-locked.  Returns after the last phase is enqueued
#define GBA_THREADS 256                                              // profiles/match_global_ba.txt: the compiler's resource report of the edge kernel and the choice
struct GbaCounters { long long launches = 0, waits = 0; };
int launch_global_ba(const GbaView& w, const int* cs, int iterations, bool robust, double* pinned, hipStream_t s, GbaDiag& dg, GbaCounters& cnt);

// Map-point upkeep (match_mappoints.hip, host/map_points.hpp).  k_tri_points: the loop of LocalMapping::CreateNewMapPoints, one lane per match over the n matches of all
// pairs of a call.  k_mp_descriptor: MapPoint::ComputeDistinctiveDescriptors, one wave per point; k_mp_normal: MapPoint::UpdateNormalAndDepth, one lane per point.
// Device pointers throughout; profiles/match_map_points.txt has the compiler's resource report
#define TRI_THREADS 64
#define MPD_THREADS 256                                              // four waves, four points
#define MPN_THREADS 64
int launch_tri_points(const TriCam& c, const TriPair* pairs, const TriMatch* matches, TriOut* out, int n, hipStream_t s);
int launch_mp_descriptor(const MpArrays& a, int nPts, hipStream_t s);
int launch_mp_normal(const MpCam& c, const MpArrays& a, int nPts, hipStream_t s);

// Vocabulary-guided searches (match_bow.hip): SearchByBoW(KeyFrame*, Frame&) and SearchForTriangulation.  Side A is the one whose entries act
// (the key frame / pKF1, capacity capLast), side B the one searched (the frame / pKF2, capacity capCur).
#define BOW_MAX_KEYS 4096                                         // keypoints per side one workgroup sorts in LDS
struct BowParams {
    float fx, fy, cx, cy, nnratio; float scale[16];
    int capA, capB, sortLen /* power of two >= every count of the call */, checkOrientation, onlyStereo;
};
struct TriPose { float Tcw2[12]; float Cw1[3]; float F12[9]; };    // per pair: rows 0..2 of pKF2's pose, pKF1's camera centre, F12 row-major

struct BowArrays {                                                // device pointers, dense [B][cap...]
    const int* nA; const int* nB; const int* nodeA; const int* nodeB;
    const uint8_t* flagsA /* by_bow: kf_valid; triangulation: has_mp1 */; const float* angA; const uint32_t* descA; const float* angB; const uint32_t* descB;
    const TriPose* pose; const float* xyA; const float* urA; const uint8_t* flagsB /* has_mp2 */; const float* xyB; const int* octB; const float* urB;      // triangulation only
    int2* sortedA; int2* sortedB; int* segStart; int* nSeg; int* nValid;       // scratch: (node, index) ascending [B][cap], first entry of every node of side A [B][capA], [B], [2][B]
    int* choice;                                                  // [B][capA]: by_bow: scratch, triangulation: match12 (output)
    int* matchOfCur; int* nmatches;                               // outputs [B][capB] (by_bow), [B]
};
int launch_match_by_bow(const BowParams& p, const BowArrays& a, int B, hipStream_t s);
int launch_match_by_bow_kf(const BowParams& p, const BowArrays& a, int B, hipStream_t s);      // SearchByBoW(pKF1, pKF2): flagsA = valid1, flagsB = valid2, choice = match12 (output)
int launch_match_for_triangulation(const BowParams& p, const BowArrays& a, int B, hipStream_t s);

// Vocabulary transform (bow_kernels.hip): descriptor -> word and node at a level, TemplatedVocabulary::transform
struct VocTree { int nNodes; const int* childStart; const int* child; const uint32_t* desc; const int* wordId; const uint8_t* stopped; };   // device pointers
int launch_voc_transform(const VocTree& tree, const uint32_t* desc /* [B][cap][8] */, const int* n, int cap, int maxN /* >= 1 */, int B, int nidLevel, int* nodeId, int* wordId, hipStream_t s);
// the same and the BowVector: weight = the nodes' weights (FP64, read for leaves), leafId = scratch [B][cap]; maxN <= BOW_MAX_KEYS; bowWord / bowValue [B][cap], nWords [B]
int launch_voc_transform_bow(const VocTree& tree, const double* weight, const uint32_t* desc, const int* n, int cap, int maxN, int B, int nidLevel, int* nodeId, int* wordId, int* leafId,
                             int* bowWord, double* bowValue, int* nWords, hipStream_t s);

// Key-frame database (bowdb_kernels.hip): one query BowVector against every slot's, L1Scoring::score in the reference's order of additions
struct BowDbArrays {                                              // device pointers
    const int* slotN /* [capSlots], -1: dead */; const int* slotWord; const double* slotValue;      // [capSlots][capWords]
    const int* qN; const int* qWord; const double* qValue;        // [Q], [Q][capWords]
    int* common; int* firstWord; float* score;                    // outputs [Q][capSlots]
};
int launch_bowdb_query(const BowDbArrays& a, int capSlots, int capWords, int Q, hipStream_t s);

}  // namespace sind
