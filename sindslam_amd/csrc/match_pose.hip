// Optimizer::PoseOptimization (reference src/Optimizer.cc:239-451), whole, in ONE launch for every item of a call: the four rounds, their ten Levenberg-Marquardt
// iterations and every trial of an iteration (OptimizationAlgorithmLevenberg::solve, optimization_algorithm_levenberg.cpp:61-164).  host/pose_opt.hpp is the one
// source of the arithmetic and of the control flow for this file and for the host twin (host/pose_opt.cpp); this file supplies the evaluator: how a workgroup
// forms g2o's sums over the edges.  The device result is compared with the host's bit for bit (tests/test_poseopt_gpu.py).
//
// Shape.  One workgroup of 192 threads per item, in the ordered sum of ordered_sum.hpp.  Waves 1 and 2 are the 128 EDGE lanes: in a chunk of 128 consecutive edges
// each computes one edge (map, error, robustify, the Jacobian, the 21 + 6 + 1 contributions of pose_opt.hpp's po_edge_contrib).  Wave 0 is the SUM wave: lane k < 28
// carries the running sum of entry k.  That is g2o's sum: H, b and the robust chi2 are cleared and every level-0 edge adds to them in edge order, each a sequential
// FP64 sum (an edge of level 1 is skipped there and skipped here).  Rows are padded to 129 doubles so the 28 sum lanes read 28 different bank pairs.
// The 6 x 6 part (LDLT, exp, the lambda logic) is not broadcast: every lane computes it from the same 28 sums, which keeps the control flow of pose_optimize
// uniform over the workgroup (all barriers are reached by all threads) and costs nothing but the lanes' idle slots.  Its small matrices are indexed dynamically
// (the pivoting) and live in scratch; profiles/match_pose_opt.txt has the compiler's report.
// KNOWN LATENCY FLOOR, UNMEASURED: the ordered sum is a serial chain of n dependent FP64 additions per linearisation (and per trial, for the chi2 alone), n LDS reads
// behind them; with up to 4 x 10 linearisations and as many or more trials a call has at most 4 x 10 x 11 such chains.  Nothing in the kernel can shorten a chain
// without changing the order of the additions, which the equality with the host forbids.
// Every loop is bounded as in the reference (4 rounds, 10 iterations, 10 trials, ceil(n / 128) + 1 chunk steps); a NaN system fails the compares that continue
// them.  No atomics, no inline assembly.  mvbOutlier (= the edge's level) is the item's row of the outlier output; it is read and written by different lanes in
// different phases, always with a barrier in between.
#include "match.hpp"
#include "ordered_sum.hpp"
#include "host/pose_opt.hpp"

namespace sind {

#define PO_THREADS 192
#define PO_CHUNK 128
#define PO_ROW 129                                                   // PO_CHUNK + 1: see above

static_assert(sizeof(PoseOptResult) == sizeof(PoseOptOut), "PoseOptResult is PoseOptOut");

struct PoseOptWg {                                                   // the evaluator of pose_optimize for one workgroup (pose_opt.hpp: Ev)
    int n, tid; const float4* pts; const float4* obs; uint8_t* outlier; PoseOptCam K;
    double (*buf)[POSEOPT_ENTRIES][PO_ROW]; double* total; int* cnt;                  // LDS: [2], [28], [PO_THREADS]

    __device__ void sums(const PoseQ& P, bool robust, bool full, double* S) {
        ordered_sums<POSEOPT_ENTRIES, PO_CHUNK, PO_ROW, PO_THREADS - PO_CHUNK>(tid, n, full ? 0 : 27 /* not full: the chi2 row alone */, buf, total,
            [&](int i, double* v) {
                if (outlier[i]) return false;                        // initializeOptimization(0): level-0 edges only
                const float4 X = pts[i], U = obs[i];
                po_edge_contrib(P, K, X.x, X.y, X.z, U.x, U.y, U.z, X.w, robust, full, v);
                return true;
            },
            [](int k) { return k >= 21 && k < 27; }, S);             // b -= ...
    }

    __device__ int classify(const PoseQ& Perr, const PoseQ& Pest) {
        int bad = 0;
        for (int i = tid; i < n; i += PO_THREADS) {
            const float4 X = pts[i], U = obs[i];
            const bool out = po_edge_is_outlier(outlier[i] ? Pest : Perr, K, X.x, X.y, X.z, U.x, U.y, U.z, X.w);
            outlier[i] = out ? 1 : 0; bad += out ? 1 : 0;
        }
        cnt[tid] = bad;
        __syncthreads();
        int nBad = 0;
        for (int t = 0; t < PO_THREADS; t++) nBad += cnt[t];
        __syncthreads();                                             // cnt[] may be rewritten by the next round's classify; the outlier flags are visible to sums()
        return nBad;
    }
};

__global__ __launch_bounds__(PO_THREADS) void k_pose_opt(PoseOptParams p, PoseOptArrays a, int B) {
    __shared__ double buf[2][POSEOPT_ENTRIES][PO_ROW];
    __shared__ double total[POSEOPT_ENTRIES];
    __shared__ int cnt[PO_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;                                              // the whole workgroup
    const int n = min(max(a.n[b], 0), p.cap);                        // the host has checked the range; never outside the item's rows
    uint8_t* outlier = a.outlier + (size_t)b * p.cap;
    for (int i = tid; i < n; i += PO_THREADS) outlier[i] = 0;         // pFrame->mvbOutlier[i] = false (:289, :323)
    __syncthreads();
    PoseOptWg ev{n, tid, a.pts + (size_t)b * p.cap, a.obs + (size_t)b * p.cap, outlier, {p.fx, p.fy, p.cx, p.cy, p.bf}, buf, total, cnt};
    float Tcw[16];
    for (int k = 0; k < 16; k++) Tcw[k] = a.Tcw[(size_t)b * 16 + k];
    PoseOptOut o;
    pose_optimize(ev, n, Tcw, o);
    if (tid == 0) {
        PoseOptResult& r = a.res[b];
        for (int k = 0; k < 16; k++) r.Tcw[k] = o.Tcw[k];
        r.nGood = o.nGood; r.nRounds = o.nRounds;
        for (int k = 0; k < 4; k++) { r.iters[k] = o.iters[k]; r.nbad[k] = o.nbad[k]; r.chi2[k] = o.chi2[k]; r.lambda[k] = o.lambda[k]; for (int j = 0; j < 12; j++) r.pose[k][j] = o.pose[k][j]; }
    }
}

int launch_pose_optimize(const PoseOptParams& p, const PoseOptArrays& a, int B, hipStream_t s) {
    if (B < 1) return SIND_OK;
    hipLaunchKernelGGL(k_pose_opt, dim3(B), dim3(PO_THREADS), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
