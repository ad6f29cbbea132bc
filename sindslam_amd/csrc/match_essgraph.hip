// Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044), whole, for every item of a call: k_ess_graph runs all 20 Levenberg-Marquardt iterations,
// every trial, every numeric linearisation, the envelope factorisation and the pose recovery in ONE launch; k_ess_points follows on the same stream without a host
// wait and corrects the map points of all items.  host/essential_graph.hpp is the one source of the arithmetic, of the order of every sum and of the control flow for
// this file and for the host twin (host/essential_graph.cpp): every phase there is a function of ONE output element (a perturbed estimate of a vertex, one of the 29
// error evaluations of an edge, one entry of an edge's Jacobians or of its blocks, one entry of a vertex's or a pair's block, one entry of a column of L, a vertex, a
// point).  This file names the executor (WgExec, match_device.hpp): the ESS_THREADS lanes of one workgroup stride over the elements of a phase, then one __syncthreads().  The device result is
// compared with the host's bit for bit (tests/test_essgraph_gpu.py).
//
// Shape.  k_ess_graph: one workgroup per item, B items per grid.  The error lanes carry the weight of a linearisation: 29 evaluations of log(C * Si * Sj^-1) per edge,
// each with its own branches of Sim3::log, so neighbouring lanes diverge inside s3_log; the values they write (7 doubles each) lie densely in the item's workspace.
// The ordered sums are one lane per entry of a block, walking the vertex's or the pair's edges in ascending order; one more lane carries the chi2 chain (ba_chain<8>).
// LDL^T: column by column over the envelope, the entries of a column spread over the lanes, each lane forming the pivot for itself (which saves the second barrier of
// a column); a column's k loop is as long as the envelope's row, not as the matrix.  The finished L(j, .) * D strip of a column is NOT staged in LDS: each lane reads
// row j and D from global memory (L2-resident: a row is at most a few KB and every lane of the column reads the same addresses, which the memory system broadcasts);
// profiles/match_essential_graph.txt has the compiler's resource report, the choice of ESS_THREADS and the timings.
// The Levenberg-Marquardt scalars are computed redundantly by every lane from the same workspace values (WgExec::rd), so every barrier is reached by all lanes.
// Every loop is bounded as in the reference: 20 iterations, 10 trials; a NaN system fails the compares that continue them.  No cooperative launch, no grid-wide flags,
// no atomics, no inline assembly.  The workspace is the item's alone; an item never reads or writes outside the regions ess_bind gave it, and every index it follows
// (edge -> key frames, list entries, envelope offsets, point -> key frame) was built or checked by the host layer before the launch.
// k_ess_points: blockIdx.y is the item, the lanes of ESS_PT_BLOCKS x ESS_PT_THREADS stride over its points; a point reads vScw and Swc of its reference key frame,
// which k_ess_graph left in the item's workspace.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

__global__ __launch_bounds__(ESS_THREADS) void k_ess_graph(const EssView* views, int B) {
    const int b = blockIdx.x;
    if (b >= B) return;                                              // the whole workgroup
    const EssView w = views[b];
    WgExec<ESS_THREADS> ex{(int)threadIdx.x};
    essential_graph(ex, w);
}

__global__ __launch_bounds__(ESS_PT_THREADS) void k_ess_points(const EssView* views, int B) {
    const int b = blockIdx.y;
    if (b >= B) return;
    const EssView& w = views[b];
    const int nMp = w.nMp;
    for (int j = blockIdx.x * ESS_PT_THREADS + threadIdx.x; j < nMp; j += gridDim.x * ESS_PT_THREADS) ess_point(w, j);
}

int launch_essential_graph(const EssView* views, int B, int maxMp, hipStream_t s) {
    if (B < 1) return SIND_OK;
    hipLaunchKernelGGL(k_ess_graph, dim3(B), dim3(ESS_THREADS), 0, s, views, B);
    HIP_TRY(hipGetLastError());
    if (maxMp > 0) {
        const int bx = std::min(ESS_PT_BLOCKS, (maxMp + ESS_PT_THREADS - 1) / ESS_PT_THREADS);
        hipLaunchKernelGGL(k_ess_points, dim3(bx, B), dim3(ESS_PT_THREADS), 0, s, views, B);
        HIP_TRY(hipGetLastError());
    }
    return SIND_OK;
}

}  // namespace sind
