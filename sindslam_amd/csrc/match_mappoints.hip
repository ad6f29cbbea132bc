// Map-point upkeep on the GPU: the per-match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:284-431), MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371).  host/map_points.hpp is the one source of the floating-point arithmetic for this file and for
// the host twins (host/map_points.cpp); the device results are compared with the host's bit for bit (tests/test_mappoints_gpu.py).
//
// k_tri_points: one lane per match over the flattened matches of all pairs of a call; nothing in the loop body depends on another match.  The per-pair constants
// (four poses) sit in a TriPair record that the lane reads through its match's pair index, the camera in kernel arguments; the 4 x 4 At and Vt and the four squared
// norms of the Jacobi SVD stay in registers (every index a constant after unrolling; profiles/match_map_points.txt has the compiler's report: no scratch).  The sweeps
// end per lane when one passes without a rotation, so the lanes of a wave diverge by a sweep or two; that is accepted.  The stereo parallax cosines arrive in TriMatch:
// atan2 and cos are the host's, never evaluated here.
//
// k_mp_descriptor: ONE WAVE PER POINT, MPD_THREADS / 64 points per workgroup.  The reference fills Distances[N][N], sorts every row and takes entry (int)(0.5 (N - 1)); here
// no matrix is stored and nothing is sorted.  Lane l holds descriptor l of the point's list in 8 registers (lists of at most 64 observations: the usual case).  For each
// row i (wave-uniform; rows of bad observers are skipped): descriptor i is read through a wave-uniform address, every lane forms its distance to it (8 xor, 8
// popcount, 7 add), and the row's median is the smallest v in 0..256 with #{d <= v} >= (int)(0.5 (N - 1)) + 1, found by bisection: at most 9 steps of one compare, one
// ballot, one 64-bit popcount and a scalar select.  Per row that is 23 vector ALU instructions for the distance and 9 vector compares; the rest is scalar.  The running
// best median and its row are wave-uniform (they derive from ballots alone); `<` keeps the first row among equals.  Lists of more than 64 observations run the same
// loop over 64-lane chunks, the ballot counts added; the chunk's descriptor is then read again in every step (from L1 / L2: a point's descriptors are 32 N bytes) and
// there is no limit on N.  Lanes beyond the list and lanes of bad observers vote 0 in every ballot; every lane of the wave reaches every ballot.
//
// k_mp_normal: one lane per point walks its own observation list: the sum is sequential FP32 in list order, and that order is the point of the kernel.
//
// No LDS, no atomics, no inline assembly.  Every index the kernels follow (point -> observations -> camera centre, ref_obs, octave) was checked by the host layer before
// the launch; lanes and waves beyond the count return before their first load.
#include "match.hpp"

namespace sind {

__global__ __launch_bounds__(TRI_THREADS) void k_tri_points(TriCam c, const TriPair* pairs, const TriMatch* matches, TriOut* out, int n) {
    const int k = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (k >= n) return;
    const TriMatch q = matches[k];
    const TriPair P = pairs[q.pair];
    TriOut o;
    tri_point(c, P, q, o);
    out[k] = o;
}

__device__ __forceinline__ int d_distance8(const uint32_t* a, const uint32_t* b) {
    int d = 0;
    for (int k = 0; k < 8; k++) d += __popc(a[k] ^ b[k]);
    return d;
}

__global__ __launch_bounds__(MPD_THREADS) void k_mp_descriptor(MpArrays a, int nPts) {
    const int lane = threadIdx.x & 63, j = (blockIdx.x * MPD_THREADS + threadIdx.x) >> 6;
    if (j >= nPts) return;                                           // the whole wave
    if (!(a.todo[j] & 1)) return;
    const int first = a.obsFirst[j], n = a.obsCount[j];
    int N = 0;                                                       // the observers that are not bad
    for (int c = 0; c < n; c += 64) { const int e = c + lane; N += __popcll(__ballot(e < n && !a.obsBad[first + (e < n ? e : 0)])); }
    if (N == 0) { if (lane == 0) a.bestObs[j] = -1; return; }        // no observations, or every observer bad: mDescriptor stays
    const int need = (int)(0.5 * (N - 1)) + 1;
    int best = 0x7fffffff, bestIdx = 0;
    if (n <= 64) {
        const bool mine = lane < n && !a.obsBad[first + (lane < n ? lane : 0)];
        uint32_t w[8];
        for (int k = 0; k < 8; k++) w[k] = mine ? a.obsDesc[8 * (size_t)(first + lane) + k] : 0u;
        for (int i = 0; i < n; i++) {
            if (a.obsBad[first + i]) continue;
            const int d = d_distance8(w, a.obsDesc + 8 * (size_t)(first + i));
            int lo = 0, hi = 256;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (__popcll(__ballot(mine && d <= mid)) >= need) hi = mid; else lo = mid + 1;
            }
            if (lo < best) { best = lo; bestIdx = i; }
        }
    } else {
        for (int i = 0; i < n; i++) {
            if (a.obsBad[first + i]) continue;
            const uint32_t* di = a.obsDesc + 8 * (size_t)(first + i);
            int lo = 0, hi = 256;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                int cnt = 0;
                for (int c = 0; c < n; c += 64) {
                    const int e = c + lane; const bool mine = e < n && !a.obsBad[first + (e < n ? e : 0)];
                    const int d = mine ? d_distance8(a.obsDesc + 8 * (size_t)(first + e), di) : 257;
                    cnt += __popcll(__ballot(d <= mid));
                }
                if (cnt >= need) hi = mid; else lo = mid + 1;
            }
            if (lo < best) { best = lo; bestIdx = i; }
        }
    }
    if (lane < 8) a.descOut[8 * (size_t)j + lane] = a.obsDesc[8 * (size_t)(first + bestIdx) + lane];
    if (lane == 0) a.bestObs[j] = bestIdx;
}

__global__ __launch_bounds__(MPN_THREADS) void k_mp_normal(MpCam c, MpArrays a, int nPts) {
    const int j = blockIdx.x * MPN_THREADS + threadIdx.x;
    if (j >= nPts) return;
    if (!(a.todo[j] & 2)) return;
    mp_normal_depth(c, a, j);
}

int launch_tri_points(const TriCam& c, const TriPair* pairs, const TriMatch* matches, TriOut* out, int n, hipStream_t s) {
    if (n < 1) return SIND_OK;
    hipLaunchKernelGGL(k_tri_points, dim3(divup(n, TRI_THREADS)), dim3(TRI_THREADS), 0, s, c, pairs, matches, out, n);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_mp_descriptor(const MpArrays& a, int nPts, hipStream_t s) {
    if (nPts < 1) return SIND_OK;
    hipLaunchKernelGGL(k_mp_descriptor, dim3(divup(nPts, MPD_THREADS / 64)), dim3(MPD_THREADS), 0, s, a, nPts);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_mp_normal(const MpCam& c, const MpArrays& a, int nPts, hipStream_t s) {
    if (nPts < 1) return SIND_OK;
    hipLaunchKernelGGL(k_mp_normal, dim3(divup(nPts, MPN_THREADS)), dim3(MPN_THREADS), 0, s, c, a, nPts);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
