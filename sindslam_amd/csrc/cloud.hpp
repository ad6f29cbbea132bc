// Mapping-consumer cloud generation interface (reference octomap_pub/src/pubPointCloud.cc:471-660); kernels in cloud_kernels.hip.
#pragma once
#include "common.hpp"

struct sind_cloud;

namespace sind {

constexpr int CLOUD_LABELS = 12, CLOUD_CHUNK = 1024;

struct CloudCam { double fx, fy, cx, cy, depthScale; };
struct CloudPose { double rel[12], twc[12]; };                    // rows 0..2 of poseRelative and of Twc, row-major
struct CloudPoint { float x, y, z; uint8_t b, g, r, a; };

struct CloudArrays {                                              // device pointers, dense per frame
    const uint8_t* bgr; const uint16_t* depth; const uint16_t* depthLast; const uint8_t* dyna; const uint8_t* dynaLast; const uint8_t* label; const CloudPose* pose;
    int* chunkCnt;        // [B][nchunks][12]  stride-2 pixels per label and chunk
    int* chunkOff;        // [B][nchunks][12]  output offset of each (chunk, label), -1 when the cluster is rejected
    int* occlusion;       // [B][12]           vecOcclusion
    int* labelCount;      // [B][12]           countNonZero(imgLabel == i), full resolution
    int* kept;            // [B][12]
    int* total;           // [B]
    CloudPoint* out;      // [B][np]
};

int launch_cloud(const CloudCam& cam, const CloudArrays& a, int W, int H, int B, hipStream_t s);
inline int cloud_grid_points(int W, int H) { return ((W + 1) / 2) * ((H + 1) / 2); }

// Statistical outlier filter of the cloud (cloud_filter.hip; the arithmetic is host/cloud_filter.hpp).
constexpr int CF_GMAX = 128;                 // cells per axis at most
constexpr int CF_CELLS = 1 << 20;            // cells per cloud at most
constexpr int CF_CAP = 1024;                 // candidate buffer of a wave, floats of LDS
constexpr int CF_RING_LIMIT = 4;             // a query that needs a ring beyond this one goes to the brute-force launch

struct CfPlan { float o[3], h, invh; int g[3], nf, degenerate, cells; };
struct CfStats { double mean, stddev, threshold; int valid, degenerate, nRing, nBrute; };        // = sind_cloud_filter_stats
struct CfArrays {                            // device pointers; per cloud b the rows start at b * np unless said otherwise
    const CloudPoint* pts; int stride;       // [B][stride]
    const int* n;                            // [B]
    int np;
    unsigned* bbox;                          // [B][6]  order-preserving codes of min x, y, z and max x, y, z over the finite points
    int* nfin;                               // [B]
    CfPlan* plan;                            // [B]
    int* cellStart;                          // [B][CF_CELLS + 1]
    int* cursor;                             // [B][CF_CELLS]   counts, then the scatter's cursors
    float4* sorted;                          // [B][np]  finite points in cell order, w = the point's index as bits
    int* list; int* listN;                   // [B][np], [B]  sorted positions of the queries left to the brute-force launch
    float* dist;                             // [B][np]
    int* chunkOff;                           // [B][nchunks]
    CfStats* stats;                          // [B]
    int* nOut;                               // [B]
    CloudPoint* out;                         // [B][np]
};
int launch_cloud_filter(const CfArrays& a, int B, int nmax, int mean_k, double stddev_mul, hipStream_t s);

// The clouds that the last sind_cloud_generate left on the device, for the other handles that read them in place (capi_occmap.cpp): rows of `stride` points,
// lastB of them (0 before any generate), their sizes in host memory.
struct CloudResident { const CloudPoint* pts; int stride, lastB, device; const int* n; };
CloudResident cloud_resident(const sind_cloud* c);

}  // namespace sind
