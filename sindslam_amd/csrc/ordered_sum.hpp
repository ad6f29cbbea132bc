// g2o's sums over the edges of a single-vertex graph (H, b and the robust chi2, each cleared and then added to by every active edge in edge order) by one workgroup,
// for k_pose_opt (match_pose.hip) and k_sim3_opt (match_sim3opt.hip).  The lanes from FIRST_EDGE_LANE on are the CHUNK edge lanes: in a chunk of CHUNK consecutive
// edges each computes one edge's ENTRIES contributions and writes them as [entry][edge] into one of two LDS buffers.  Lane k < ENTRIES of wave 0 carries the running
// sum of entry k and adds the previous chunk's values in ascending edge order meanwhile, from the other buffer; one barrier per chunk.  Every S[k] is therefore the
// sequential FP64 sum from 0 that the host twin's plain loop forms.  Rows are padded to ROW = CHUNK + 1 doubles so that the sum lanes read different bank pairs.
// The workgroup has exactly FIRST_EDGE_LANE + CHUNK threads (the kernels' __launch_bounds__ and their launches), so an edge lane's column lies inside a row.
// Every lane of the workgroup calls this with the same arguments: it passes ceil(nEdges / CHUNK) + 2 barriers, and on return every lane holds all the sums.
#pragma once
#include <hip/hip_runtime.h>

namespace sind {

// first:           the first row wanted (a trial wants the chi2 row alone); S[k] = 0 below it
// edge(i, v):      -> is edge i active; if so v[first .. ENTRIES - 1] are its contributions.  An inactive edge adds 0: x + 0 = x - 0 = x for every x these sums can
//                  hold (never -0)
// subtracts(k):    row k is subtracted from its sum, not added (pose: the b rows, b -= ...)
// buf, total:      LDS, [2][ENTRIES][ROW] and [ENTRIES].  The caller's next write to either must come after a barrier of its own that follows this call's reads of
//                  total[]; the next call's own first write does: it comes after that call's first barrier, which a lane reaches only after these reads
template <int ENTRIES, int CHUNK, int ROW, int FIRST_EDGE_LANE, class Edge, class Subtracts>
__device__ __forceinline__ void ordered_sums(int tid, int nEdges, int first, double (*buf)[ENTRIES][ROW], double* total, Edge edge, Subtracts subtracts, double* S) {
    static_assert(ROW > CHUNK, "a row holds a chunk");
    const int nChunks = (nEdges + CHUNK - 1) / CHUNK;
    double run = 0.0;
    for (int c = 0; c <= nChunks; c++) {
        if (tid >= FIRST_EDGE_LANE && c < nChunks) {                 // edge lanes: chunk c into buffer c & 1
            const int e = tid - FIRST_EDGE_LANE, i = c * CHUNK + e;
            if (i < nEdges) {
                double v[ENTRIES];
                const bool active = edge(i, v);
                double (*B)[ROW] = buf[c & 1];
                for (int k = first; k < ENTRIES; k++) B[k][e] = active ? v[k] : 0.0;
            }
        }
        if (tid >= first && tid < ENTRIES && c > 0) {                // sum lanes: chunk c - 1 from the other buffer
            const int m = min(CHUNK, nEdges - (c - 1) * CHUNK);
            const double* row = buf[(c - 1) & 1][tid];
            if (subtracts(tid)) { for (int j = 0; j < m; j++) run = run - row[j]; }
            else { for (int j = 0; j < m; j++) run = run + row[j]; }
        }
        __syncthreads();
    }
    if (tid >= first && tid < ENTRIES) total[tid] = run;
    __syncthreads();
    for (int k = 0; k < ENTRIES; k++) S[k] = k >= first ? total[k] : 0.0;
}

}  // namespace sind
