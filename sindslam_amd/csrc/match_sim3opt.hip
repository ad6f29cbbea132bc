// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1046-1241), whole, in ONE launch for every item of a call: both stages, their Levenberg-Marquardt iterations,
// every trial of an iteration and the two classifications.  host/sim3_opt.hpp is the one source of the arithmetic and of the control flow for this file and for the
// host twin (host/sim3_opt.cpp); this file supplies the evaluator: how a workgroup forms g2o's sums over the edges.  The device result is compared with the host's
// bit for bit (tests/test_sim3opt_gpu.py).
//
// Shape.  One workgroup of 128 threads per item.  A pair has two edges, edge 2 i the EdgeSim3ProjectXYZ of pair i and edge 2 i + 1 its EdgeInverseSim3ProjectXYZ: the
// order of g2o's active edges.  The sums are the ordered sum of ordered_sum.hpp: wave 1 is the 64 EDGE lanes, in a chunk of 64 consecutive edges each computes one
// edge (its error, the Huber weight, the numeric Jacobian from 14 more error evaluations, the 28 + 7 + 1 contributions of sim3_opt.hpp's s3_edge_contrib); wave 0 is
// the SUM wave: lane k < 36 carries the running sum of entry k.  Rows are padded to 65 doubles; two buffers of 36 x 65 doubles are 37440 B, inside the 64 KB a
// kernel gets without asking.
// The 15 transforms of a linearisation (the estimate and its 14 perturbations, each with its inverse) are the same for every edge: lanes 0..14 form one each into
// LDS before the chunks start, and the edge lanes read them from there (a broadcast read).  A trial needs the estimate and its inverse only: lane 0.
// The 7 x 7 part (LDLT, the Sim3 exponential, the lambda logic) is not broadcast: every lane computes it from the same 36 sums, which keeps the control flow of
// sim3_optimize uniform over the workgroup (all barriers are reached by all threads).  profiles/match_sim3_opt.txt has the compiler's report.
// LATENCY FLOOR: the ordered sum is a serial chain of 2 n dependent FP64 additions per linearisation and per trial, an LDS read behind each.  Nothing in the kernel can
// shorten it without changing the order of the additions, which the equality with the host forbids.
// Every loop is bounded as in the reference (2 stages, 5 or 10 iterations, 10 trials, ceil(2 n / 64) + 1 chunk steps); a NaN system fails the compares that continue
// them.  No atomics, no inline assembly.  removed[] is the item's row of the output and the kernel's working state; it is read and written by different lanes in
// different phases, always with a barrier in between.
#include "match.hpp"
#include "ordered_sum.hpp"
#include "host/sim3_opt.hpp"

namespace sind {

#define SO_THREADS 128
#define SO_CHUNK 64
#define SO_ROW 65                                                    // SO_CHUNK + 1: see above

static_assert(sizeof(Sim3OptResult) == sizeof(Sim3OptOut), "Sim3OptResult is Sim3OptOut");

struct Sim3OptWg {                                                   // the evaluator of sim3_optimize for one workgroup (sim3_opt.hpp: Ev)
    int n, tid; const float4* p1; const float4* p2; const float4* ob; uint8_t* removed; Sim3Cam K1, K2; float th2; double delta; bool fixScale;
    double (*buf)[SIM3OPT_ENTRIES][SO_ROW]; Sim3Q (*T)[SIM3OPT_TRANSFORMS]; double* total; int* cnt;   // LDS: [2], [2] (forward, inverse), [36], [2][SO_THREADS]

    __device__ void sums(const Sim3Q& est, bool full, double* S) {
        if (tid < (full ? SIM3OPT_TRANSFORMS : 1)) { Sim3Q a, b; s3_perturbed(est, tid, fixScale, a, b); T[0][tid] = a; T[1][tid] = b; }
        __syncthreads();
        ordered_sums<SIM3OPT_ENTRIES, SO_CHUNK, SO_ROW, SO_THREADS - SO_CHUNK>(tid, 2 * n, full ? 0 : 35 /* not full: the chi2 row alone */, buf, total,
            [&](int k, double* v) {
                const int i = k >> 1, side = k & 1;
                if (removed[i]) return false;                        // optimizer.removeEdge(e12), removeEdge(e21)
                const float4 X = side ? p1[i] : p2[i], P = side ? p2[i] : p1[i], U = ob[i];               // e12: the point of camera 2, obs1 and sigma of camera 1
                s3_edge_contrib(T[side], side ? K2 : K1, X.x, X.y, X.z, side ? U.z : U.x, side ? U.w : U.y, P.w, delta, full, v);
                return true;
            },
            [](int) { return false; }, S);                           // every row is added: b += ...
        __syncthreads();                                             // the next call writes T[] before its first barrier: only after every lane has read total[] and T[]
    }

    __device__ int classify(const Sim3Q& Serr, int* nIn) {
        Sim3Q Sinv; s3_inverse(Serr, Sinv);
        int bad = 0, in = 0;
        for (int i = tid; i < n; i += SO_THREADS) {
            if (removed[i]) continue;
            const float4 A = p1[i], B = p2[i], U = ob[i];
            const float X1[3] = {A.x, A.y, A.z}, X2[3] = {B.x, B.y, B.z}, o1[2] = {U.x, U.y}, o2[2] = {U.z, U.w};
            if (s3_pair_is_bad(Serr, Sinv, K1, K2, X1, X2, o1, o2, A.w, B.w, th2)) { removed[i] = 1; bad++; } else in++;
        }
        cnt[tid] = bad; cnt[SO_THREADS + tid] = in;
        __syncthreads();
        int nBad = 0, nI = 0;
        for (int t = 0; t < SO_THREADS; t++) { nBad += cnt[t]; nI += cnt[SO_THREADS + t]; }
        __syncthreads();                                             // cnt[] may be rewritten by the next classify; the removed flags are visible to sums()
        *nIn = nI;
        return nBad;
    }
};

__global__ __launch_bounds__(SO_THREADS) void k_sim3_opt(Sim3OptParams p, Sim3OptArrays a, int B) {
    __shared__ double buf[2][SIM3OPT_ENTRIES][SO_ROW];
    __shared__ Sim3Q T[2][SIM3OPT_TRANSFORMS];
    __shared__ double total[SIM3OPT_ENTRIES];
    __shared__ int cnt[2 * SO_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;                                              // the whole workgroup
    const Sim3OptHead h = a.head[b];
    const int n = min(max(h.n, 0), p.cap);                           // the host has checked the range; never outside the item's rows
    uint8_t* removed = a.removed + (size_t)b * p.cap;
    for (int i = tid; i < n; i += SO_THREADS) removed[i] = 0;
    __syncthreads();
    Sim3OptWg ev{n, tid, a.p1 + (size_t)b * p.cap, a.p2 + (size_t)b * p.cap, a.ob + (size_t)b * p.cap, removed,
                 {(double)h.K1[0], (double)h.K1[1], (double)h.K1[2], (double)h.K1[3]}, {(double)h.K2[0], (double)h.K2[1], (double)h.K2[2], (double)h.K2[3]},
                 p.th2, s3_delta(p.th2), p.fixScale != 0, buf, T, total, cnt};
    Sim3Q S0; s3_from_input(h.s12, h.R12, h.t12, S0);
    Sim3OptOut o;
    sim3_optimize(ev, n, S0, p.fixScale != 0, o);
    if (tid == 0) {
        Sim3OptResult& r = a.res[b];
        for (int k = 0; k < 4; k++) r.q[k] = o.q[k];
        for (int k = 0; k < 3; k++) r.t[k] = o.t[k];
        r.s = o.s; r.nIn = o.nIn; r.nBad = o.nBad; r.stages = o.stages;
        for (int k = 0; k < 2; k++) { r.iters[k] = o.iters[k]; r.chi2[k] = o.chi2[k]; r.lambda[k] = o.lambda[k]; }
    }
}

int launch_sim3_optimize(const Sim3OptParams& p, const Sim3OptArrays& a, int B, hipStream_t s) {
    if (B < 1) return SIND_OK;
    hipLaunchKernelGGL(k_sim3_opt, dim3(B), dim3(SO_THREADS), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
