// Optimizer::BundleAdjustment (reference src/Optimizer.cc:49-237), the optimize of a global bundle adjustment, as PHASES OVER THE WHOLE GRID.  host/ba_schur.hpp (the
// phases local BA has too) and host/global_ba.hpp (the envelope, the control flow) are the one source of the arithmetic and of the order of every sum for this file and
// for the host twin (host/global_ba.cpp): every phase there is
// a named function of ONE output element (an edge, one entry of one vertex's Hessian block, one entry of an upper block of Hschur, one entry of the factor, a point, a
// vertex) wrapped in a functor.  This file names the runner: run.go(n, phase) is one launch of k_gba_phase<Phase>, ceil(n / GBA_THREADS) workgroups of GBA_THREADS
// lanes, one element per lane, `if (idx < n)`; the grids are not capped.  The device result is compared with the host's bit for bit (tests/test_globalba_gpu.py).
//
// Why not local BA's shape.  k_local_ba runs an item in one workgroup, and at B = 1 that workgroup walks its chains on an otherwise empty card
// (profiles/match_local_ba.txt).  A global BA is always one item, of hundreds of key frames and about 10^5 observations, so its parallel phases are as wide as their
// element counts here: edge evaluation one lane per observation; the ordered sums one lane per entry of a vertex's block; Dinv and db per point, BDinv per edge; the
// Schur complement one lane per entry of an upper block and one per entry of coefficients; back-substitution per point, update per vertex, computeScale's terms per
// entry of x.  THE SERIAL CHAINS KEEP THEIR ORDER and are the known floor: one lane carries the chi2 chain over rho[0] laid out densely (ba_chain<32>: 32 loads in flight), in the same launch
// as the vertex sums; one lane carries computeScale's chain; one lane the max diagonal, once per call.
// The factorisation of the reduced camera system (a natural-order envelope in 6 x 6 block rows) costs at most three launches per block column, never one per scalar
// column: every stored entry of the block column takes its terms left of the column, one lane finishes the diagonal block, every row below finishes inside the column.
// The two triangular solves are ONE launch of ONE workgroup that walks the columns with barriers (WgExec, as k_local_ba does).
//
// Synchronisation.  Stream order between the launches, __syncthreads() inside the one-workgroup solve; nothing else: no cooperative launch, no grid-wide flags or
// spins, no atomics, no inline assembly.  The Levenberg-Marquardt driver (host/g2o_lm.hpp) runs on the host; its scalars come back through one page-locked buffer:
// one wait per linearisation (chi2 and, the first time, the max diagonal), one wait per trial (the fail flag, the trial's chi2 and computeScale); pop is enqueued
// without a wait.  Every index a lane follows (edge -> key frame, point, list entries, envelope offsets) was built or checked by the host layer before the first
// launch, and an edge index meets LBA_C only as size_t.  profiles/match_global_ba.txt has the compiler's resource report, the choice of GBA_THREADS and the timings.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

template <class Ph> __global__ __launch_bounds__(GBA_THREADS) void k_gba_phase(const Ph ph, int n) {
    const int idx = blockIdx.x * GBA_THREADS + threadIdx.x;
    if (idx < n) ph(idx);
}

__global__ __launch_bounds__(GBA_THREADS) void k_gba_trisolve(const GbaView w) {
    WgExec<GBA_THREADS> ex{(int)threadIdx.x};
    gba_trisolve(ex, w);
}

// run.go / run.tri / run.fetch of global_ba.hpp on a stream.  The first error stops every later launch and is what the call returns
struct GbaDevRun {
    hipStream_t s; double* pinned; GbaCounters* cnt; hipError_t err = hipSuccess;
    template <class Ph> void go(int n, const Ph& ph) {
        if (n < 1 || err != hipSuccess) return;
        hipLaunchKernelGGL(k_gba_phase<Ph>, dim3((unsigned)divup(n, GBA_THREADS)), dim3(GBA_THREADS), 0, s, ph, n);
        err = hipGetLastError(); cnt->launches++;
    }
    void tri(const GbaView& w) {
        if (err != hipSuccess) return;
        hipLaunchKernelGGL(k_gba_trisolve, dim3(1), dim3(GBA_THREADS), 0, s, w);
        err = hipGetLastError(); cnt->launches++;
    }
    void fetch(const GbaView& w, double* sc) {
        for (int k = 0; k < BA_SC_N; k++) sc[k] = 0.0;
        if (err == hipSuccess) err = hipMemcpyAsync(pinned, w.sc, BA_SC_N * sizeof(double), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        cnt->waits++;
        if (err == hipSuccess) for (int k = 0; k < BA_SC_N; k++) sc[k] = pinned[k];
        else sc[BA_SC_CHI] = NAN;                                   // ends the driver's loops: every compare that continues them fails
    }
};

int launch_global_ba(const GbaView& w, const int* cs, int iterations, bool robust, double* pinned, hipStream_t s, GbaDiag& dg, GbaCounters& cnt) {
    GbaDevRun run{s, pinned, &cnt};
    global_ba(run, w, cs, iterations, robust, dg);
    HIP_TRY(run.err);
    return SIND_OK;
}

}  // namespace sind
