// Projection matcher interface (reference src/ORBmatcher.cc:45-129, :1328-1470, :1472-1599); kernels in match_kernels.hip, match_local.hip.
#pragma once
#include "common.hpp"

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

// reloc = 0: Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th); reloc = 1: SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
int launch_project_points(const LocalParams& p, const LocalArrays& a, int B, int reloc, hipStream_t s);
int launch_search_points(const LocalParams& p, const LocalArrays& a, int B, int reloc, hipStream_t s);

}  // namespace sind
