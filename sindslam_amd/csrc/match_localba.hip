// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:506-778), whole, in ONE launch for every item of a call: both stages, their five and ten
// Levenberg-Marquardt iterations, every trial of an iteration, the Schur complement, the factorisation of the reduced camera system and both classifications.
// host/ba_schur.hpp (the phases global BA has too) and host/local_ba.hpp (the levels, the dense factor, the control flow) are the one source of the arithmetic and of
// the order of every sum for this file and for the host twin (host/local_ba.cpp):
// every phase there is a function of ONE output element (an edge, one entry of one vertex's Hessian block, one entry of an upper block of Hschur, one entry of a column
// of L, a point, a vertex).  This file names the executor (WgExec, match_device.hpp): the LBA_THREADS lanes of one workgroup stride over the elements of a phase, then one __syncthreads().
// The device result is compared with the host's bit for bit (tests/test_localba_gpu.py).
//
// Shape.  One workgroup per item, B items per grid.  Edge lanes: all lanes stride over the edges; each computes its error, rho, both Jacobians and its 21 + 6 (pose),
// 6 + 3 (point), 18 (Hpl) contributions and rho[0] into the item's workspace in global memory (L2-resident for a typical window).  Ordered sums: one lane per (vertex,
// entry) walks that vertex's edges in ascending order (poses through the per-pose list the host layer builds, four edges fetched ahead of their additions; points
// contiguous in the item); one more lane carries the chi2 chain meanwhile, over rho[0] laid out densely by the edge lanes (ba_chain<8>: eight loads ahead of eight
// additions, so the chain waits for the adder and not for memory).  computeScale's terms are formed by all lanes and added by one in the same way.  Schur: one lane per entry of an upper block (i1, i2) and one per entry of coefficients, each walking the points both poses see in ascending
// point order.  LDL^T: column by column, the entries of a column spread over the lanes (each lane forms the pivot for itself, which saves the second barrier of a
// column).  Back-substitution, update and classification: spread over the lanes by point, vertex or edge.
// The Levenberg-Marquardt scalars are computed redundantly by every lane from the same workspace values (WgExec::rd), so every barrier is reached by all lanes.
// KNOWN LATENCY FLOOR: the chi2 chain is one dependent FP64 add per edge per evaluation and a pose's chains one per edge of that pose; more lanes cannot shorten a
// chain whose order is fixed.  profiles/match_local_ba.txt has the compiler's resource report, the choice of LBA_THREADS and the timings.
// Every loop is bounded as in the reference: 2 stages, 5 and 10 iterations, 10 trials; a NaN system fails the compares that continue them.  No cooperative launch, no
// grid-wide flags, no atomics, no inline assembly.  The workspace is the item's alone; an item never reads or writes outside the regions lba_bind gave it, and every
// index it follows (edge -> key frame, point, list entries) was built or checked by the host layer before the launch.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

__global__ __launch_bounds__(LBA_THREADS) void k_local_ba(const LbaView* views, int B) {
    const int b = blockIdx.x;
    if (b >= B) return;                                              // the whole workgroup
    const LbaView w = views[b];
    WgExec<LBA_THREADS> ex{(int)threadIdx.x};
    local_ba(ex, w);
}

int launch_local_ba(const LbaView* views, int B, hipStream_t s) {
    if (B < 1) return SIND_OK;
    hipLaunchKernelGGL(k_local_ba, dim3(B), dim3(LBA_THREADS), 0, s, views, B);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
