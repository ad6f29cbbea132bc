// Statistical outlier filter of the key-frame cloud on the GPU (reference octomap_pub/src/pubPointCloud.cc:291-296, pcl::StatisticalOutlierRemoval; the contract and
// its arithmetic are host/cloud_filter.hpp, parity with a real PCL / FLANN build unpinned).  All B clouds run in the same launches:
//   k_cf_init, k_cf_bbox   bounding box of the finite points (min / max on order-preserving codes: exact, order independent) and their count
//   k_cf_plan              one lane per cloud: the grid.  One cell size h for the three axes, about half a point per cell of the box (the clouds of a depth camera
//                          are surfaces: an occupied cell then holds some tens of points), eight per cell where the box is flat in an axis; at most CF_GMAX cells per
//                          axis and CF_CELLS in all, so a point a kilometre away coarsens the grid and allocates nothing.  A box that is a point, of non-finite
//                          extent, or with h below 1e-15 gets ONE cell.  Fewer than mean_k + 1 finite points: degenerate, nothing else runs for that cloud.
//   k_cf_count, k_cf_scan, k_cf_scatter   counting sort of the finite points by cell key (z, y, x: a run of cells along x is one contiguous range)
//   k_cf_search            one wave per finite point, in cell order.  Ring R = 0, 1, .. CF_RING_LIMIT: the cells of Chebyshev distance R are streamed (a table of row
//                          ranges, one lane per row of cells, then 64 candidates per step); the wave keeps the mean_k + 1 smallest squared distances seen so far in a
//                          CF_CAP-float LDS buffer: candidates below the current (mean_k + 1)-th smallest T are appended by ballot rank, and a full buffer is cut back
//                          to the mean_k + 1 smallest.  T is found without sorting: bisection on the bit pattern of the non-negative floats (31 steps of compares on
//                          16 registers per lane and a wave sum), the idiom of k_mp_descriptor's median; the copies of T are made up from its count.
//                          The search stops after ring R if the box covers the grid, or if T <= bound(R); else after CF_RING_LIMIT the query goes on a list.
//   k_cf_brute             the same wave routine over ALL finite points for the listed queries (isolated points and small far clusters: what the filter is for)
//   k_cf_stats             one block per cloud: lane 0 runs the contract's ordered FP64 chain over the distances (staged through LDS 1024 at a time), then the block
//                          counts the kept points per chunk of 1024 for the stable compaction.  On the device because the alternative -- download the distances, run
//                          the twin's loop, upload the threshold -- costs a third host wait per call for a chain of ~0.3 ms at 76 800 points.
//   k_cf_compact           stable scatter by ballot rank, as k_cloud_scatter.
// Ten launches and one memset whatever B; the host waits twice (capi_cloud.cpp).
//
// bound(R), and why it is conservative.  The cell index of coordinate v on an axis is min(g - 1, trunc(t')), t' = fl(fl(v - o) * fl(1 / h)), o the box minimum: three
// roundings, so t' = t (1 + e), |e| < 2^-22, against the real t = (v - o) / h; indices stay below 128, so |t' - t| < 2^-15 cells.  Every step is monotone in v.  A point
// outside the box of radius R around the query's cell c has on some axis an index >= c + R + 1, so t'_j >= c + R + 1, or <= c - R - 1 (unclamped), so t'_j < c - R; the
// query has c <= t'_q (and t'_q < c + 1 unless c is the clamped last cell, above which there is nothing).  In reals the two are therefore more than R - 2^-14 cells
// apart on that axis: |x_q - x_j| > h (R - 2^-14).  The contract's distance is fl(fl(fl(dx^2) + fl(dy^2)) + fl(dz^2)) with dx = fl(x_q - x_j): adding non-negative
// terms never lowers a rounded sum, and fl(dx)^2 rounded twice loses less than 2^-22 relatively (h > 1e-15 keeps it far from underflow).  bound(R) = (h (R - 1/64))^2
// (1 - 2^-20) in FP64 for R >= 1 is below all of that with margin to spare, and bound(0) = 0: ring 0 alone suffices only when T is 0 (mean_k + 1 coincident points).
// T <= bound means no point outside has a smaller distance, and one at exactly T would not change the multiset.
//
// Bounds: positions in `sorted` are below nf <= n <= np, cell keys below cells <= CF_CELLS (indices are clamped per axis), cellStart has CF_CELLS + 1 entries, list
// entries below nf; the host layer checks n <= np before anything is launched.  No inline assembly; the only atomics are integer adds and unsigned min / max.
#include <algorithm>
#include "cloud.hpp"
#include "host/cloud_filter.hpp"

namespace sind {

constexpr int CF_SLOTS = CF_CAP / 64, CF_CHUNK = 1024;

__device__ __forceinline__ unsigned d_cf_code(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float d_cf_decode(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }
__device__ __forceinline__ int d_cf_axis(float v, float o, float invh, int g) { return (int)fminf((v - o) * invh, (float)(g - 1)); }      // fminf drops a NaN (one-cell grids)
__device__ __forceinline__ int d_cf_key(const CfPlan& P, float x, float y, float z) {
    return (d_cf_axis(z, P.o[2], P.invh, P.g[2]) * P.g[1] + d_cf_axis(y, P.o[1], P.invh, P.g[1])) * P.g[0] + d_cf_axis(x, P.o[0], P.invh, P.g[0]);
}
__device__ __forceinline__ int d_wave_sum(int v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }

__global__ void k_cf_init(CfArrays a) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 6) a.bbox[6 * b + t] = t < 3 ? 0xffffffffu : 0u;
    if (t == 6) a.nfin[b] = 0;
    if (t == 7) a.listN[b] = 0;
}

__global__ __launch_bounds__(256) void k_cf_bbox(CfArrays a) {
    const int b = blockIdx.y, n = a.n[b], lo = blockIdx.x * CF_CHUNK, hi = min(n, lo + CF_CHUNK);
    if (lo >= n) return;
    const CloudPoint* p = a.pts + (size_t)b * a.stride;
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}; int cnt = 0;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const float x = p[i].x, y = p[i].y, z = p[i].z;
        if (!cf_finite(x, y, z)) continue;
        const unsigned c[3] = {d_cf_code(x), d_cf_code(y), d_cf_code(z)};
        for (int k = 0; k < 3; k++) { mn[k] = min(mn[k], c[k]); mx[k] = max(mx[k], c[k]); }
        cnt++;
    }
    for (int o = 32; o; o >>= 1) {
        for (int k = 0; k < 3; k++) { mn[k] = min(mn[k], (unsigned)__shfl_xor((int)mn[k], o)); mx[k] = max(mx[k], (unsigned)__shfl_xor((int)mx[k], o)); }
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        for (int k = 0; k < 3; k++) { atomicMin(&a.bbox[6 * b + k], mn[k]); atomicMax(&a.bbox[6 * b + 3 + k], mx[k]); }
        atomicAdd(&a.nfin[b], cnt);
    }
}

__global__ void k_cf_plan(CfArrays a, int k1) {
    const int b = blockIdx.x;
    if (threadIdx.x) return;
    CfPlan P; P.nf = a.nfin[b]; P.degenerate = P.nf < k1; P.h = 1.0f; P.invh = 0.0f;
    float ext[3];
    for (int k = 0; k < 3; k++) { P.g[k] = 1; P.o[k] = P.nf ? d_cf_decode(a.bbox[6 * b + k]) : 0.0f; ext[k] = P.nf ? d_cf_decode(a.bbox[6 * b + 3 + k]) - P.o[k] : 0.0f; }
    if (!P.degenerate) {
        bool ok = true; int dims = 0; double vol = 1.0, emax = 0.0;
        for (int k = 0; k < 3; k++) { if (!isfinite(ext[k])) ok = false; if (ext[k] > 0.0f) { dims++; vol *= (double)ext[k]; emax = fmax(emax, (double)ext[k]); } }
        if (ok && dims > 0) {
            const double h0 = fmax(pow(vol * (dims == 3 ? 0.5 : 8.0) / (double)P.nf, 1.0 / dims), emax / (CF_GMAX - 0.5));
            float h = (float)h0;
            while (h > 1e-15f && isfinite(h)) {
                const float invh = 1.0f / h; int g[3];
                for (int k = 0; k < 3; k++) g[k] = ext[k] > 0.0f ? (int)fminf(ext[k] * invh, (float)(CF_GMAX - 1)) + 1 : 1;
                if ((long long)g[0] * g[1] * g[2] <= CF_CELLS) { P.h = h; P.invh = invh; for (int k = 0; k < 3; k++) P.g[k] = g[k]; break; }
                h *= 1.25f;
            }
        }
    }
    P.cells = P.g[0] * P.g[1] * P.g[2];
    a.plan[b] = P;
}

__global__ __launch_bounds__(256) void k_cf_count(CfArrays a) {
    const int b = blockIdx.y, n = a.n[b], lo = blockIdx.x * CF_CHUNK, hi = min(n, lo + CF_CHUNK);
    if (lo >= n) return;
    const CfPlan P = a.plan[b];
    const CloudPoint* p = a.pts + (size_t)b * a.stride;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        a.dist[(size_t)b * a.np + i] = 0.0f;                          // non-finite points and degenerate clouds keep it
        const float x = p[i].x, y = p[i].y, z = p[i].z;
        if (P.degenerate || !cf_finite(x, y, z)) continue;
        atomicAdd(&a.cursor[(size_t)b * CF_CELLS + d_cf_key(P, x, y, z)], 1);
    }
}

__global__ __launch_bounds__(1024) void k_cf_scan(CfArrays a) {
    __shared__ int part[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    const CfPlan P = a.plan[b];
    if (P.degenerate) return;
    int* cur = a.cursor + (size_t)b * CF_CELLS; int* start = a.cellStart + (size_t)b * (CF_CELLS + 1);
    const int per = (P.cells + 1023) / 1024, lo = min(P.cells, t * per), hi = min(P.cells, lo + per);
    int s = 0;
    for (int i = lo; i < hi; i++) s += cur[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) { const int v = t >= o ? part[t - o] : 0; __syncthreads(); part[t] += v; __syncthreads(); }
    int r = part[t] - s;                                              // exclusive
    for (int i = lo; i < hi; i++) { const int c = cur[i]; start[i] = r; cur[i] = r; r += c; }
    if (t == 1023) start[P.cells] = part[1023];
}

__global__ __launch_bounds__(256) void k_cf_scatter(CfArrays a) {
    const int b = blockIdx.y, n = a.n[b], lo = blockIdx.x * CF_CHUNK, hi = min(n, lo + CF_CHUNK);
    if (lo >= n) return;
    const CfPlan P = a.plan[b];
    if (P.degenerate) return;
    const CloudPoint* p = a.pts + (size_t)b * a.stride;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const float x = p[i].x, y = p[i].y, z = p[i].z;
        if (!cf_finite(x, y, z)) continue;
        const int pos = atomicAdd(&a.cursor[(size_t)b * CF_CELLS + d_cf_key(P, x, y, z)], 1);      // the order inside a cell is free: results are functions of multisets
        a.sorted[(size_t)b * a.np + pos] = make_float4(x, y, z, __int_as_float(i));
    }
}

// ---- the wave's running selection: buf[0 .. cnt) holds the k1 smallest squared distances seen so far (all of them while fewer than CF_CAP were seen) ----
struct CfSel { float* buf; int cnt; float T; bool haveT; int k1; };      // every field is wave-uniform

// cut buf[0 .. cnt), cnt >= k1, back to its k1 smallest; T = the k1-th smallest.  One wave per block: __syncthreads is the wave's own barrier.
__device__ void d_cf_reduce(CfSel& s, int lane) {
    __syncthreads();
    unsigned r[CF_SLOTS];
#pragma unroll
    for (int j = 0; j < CF_SLOTS; j++) { const int i = j * 64 + lane; r[j] = i < s.cnt ? __float_as_uint(s.buf[i]) : 0xffffffffu; }
    unsigned v = 0; const int rank = s.k1 - 1;                          // the value at sorted index rank = the largest v with #{x < v} <= rank
    for (int bit = 30; bit >= 0; bit--) {
        const unsigned t = v | (1u << bit); int c = 0;
#pragma unroll
        for (int j = 0; j < CF_SLOTS; j++) c += r[j] < t;
        if (d_wave_sum(c) <= rank) v = t;
    }
    int w = 0;
#pragma unroll
    for (int j = 0; j < CF_SLOTS; j++) {
        const bool keep = r[j] < v; const unsigned long long m = __ballot(keep);
        if (keep) s.buf[w + __popcll(m & ((1ull << lane) - 1ull))] = __uint_as_float(r[j]);
        w += __popcll(m);
    }
    const float T = __uint_as_float(v);
    for (int i = w + lane; i < s.k1; i += 64) s.buf[i] = T;            // w <= rank: the copies of T that belong to the k1 smallest
    s.cnt = s.k1; s.T = T; s.haveT = true;
    __syncthreads();
}

__device__ __forceinline__ void d_cf_push(CfSel& s, bool ok, float d, int lane) {
    ok = ok && (!s.haveT || d < s.T);
    unsigned long long m = __ballot(ok);
    if (!m) return;
    if (s.cnt + __popcll(m) > CF_CAP) { d_cf_reduce(s, lane); ok = ok && d < s.T; m = __ballot(ok); }      // cnt > CF_CAP - 64 >= k1 here
    if (ok) s.buf[s.cnt + __popcll(m & ((1ull << lane) - 1ull))] = d;
    s.cnt += __popcll(m);
}

__device__ __forceinline__ void d_cf_stream(CfSel& s, const float4* sp, int s0, int e0, const float4& me, int lane) {
    for (int p0 = s0; p0 < e0; p0 += 64) {
        const int p = p0 + lane; const bool ok = p < e0; float d = 0.0f;
        if (ok) { const float4 o = sp[p]; d = cf_dist2(me.x, me.y, me.z, o.x, o.y, o.z); }
        d_cf_push(s, ok, d, lane);
    }
}

// the mean distance from the selection (cnt >= k1): order the k1 survivors by rank (at most 129: three per lane), drop the first, sum the roots in order
__device__ float d_cf_finish(CfSel& s, int lane) {
    if (s.cnt > s.k1) d_cf_reduce(s, lane); else __syncthreads();
    float* srt = s.buf + 256; double* root = (double*)(s.buf + 512);
    const int k1 = s.k1;
    for (int i = lane; i < k1; i += 64) {
        const float v = s.buf[i]; int rk = 0;
        for (int j = 0; j < k1; j++) { const float u = s.buf[j]; rk += (u < v) || (u == v && j < i); }
        srt[rk] = v;
    }
    __syncthreads();
    for (int i = lane; i < k1 - 1; i += 64) root[i] = cf_root(srt[i + 1]);
    __syncthreads();
    return cf_mean_distance([&](int i) { return root[i]; }, k1 - 1);      // every lane runs the same chain on broadcast reads
}

__global__ __launch_bounds__(64) void k_cf_search(CfArrays a, int k1) {
    __shared__ __align__(16) float buf[CF_CAP];
    const int b = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
    const CfPlan P = a.plan[b];
    if (P.degenerate || q >= P.nf) return;
    const float4* sp = a.sorted + (size_t)b * a.np; const int* cs = a.cellStart + (size_t)b * (CF_CELLS + 1);
    const float4 me = sp[q];
    const int c0 = d_cf_axis(me.x, P.o[0], P.invh, P.g[0]), c1 = d_cf_axis(me.y, P.o[1], P.invh, P.g[1]), c2 = d_cf_axis(me.z, P.o[2], P.invh, P.g[2]);
    CfSel s{buf, 0, 0.0f, false, k1};
    bool done = false;
    for (int R = 0; R <= CF_RING_LIMIT && !done; R++) {
        const int side = 2 * R + 1, nr = side * side;
        for (int base = 0; base < nr; base += 64) {
            const int r = base + lane; int sA = 0, eA = 0, sB = 0, eB = 0;      // the ranges of row r of the ring: a face row is one run of cells, an inner row two cells
            if (r < nr) {
                const int dz = r / side - R, dy = r % side - R, z = c2 + dz, y = c1 + dy;
                if (z >= 0 && z < P.g[2] && y >= 0 && y < P.g[1]) {
                    const int row = (z * P.g[1] + y) * P.g[0], xl = c0 - R, xh = c0 + R;
                    if (abs(dz) == R || abs(dy) == R) { sA = cs[row + max(xl, 0)]; eA = cs[row + min(xh, P.g[0] - 1) + 1]; }
                    else { if (xl >= 0) { sA = cs[row + xl]; eA = cs[row + xl + 1]; } if (xh < P.g[0]) { sB = cs[row + xh]; eB = cs[row + xh + 1]; } }
                }
            }
            const int lim = min(64, nr - base);
            for (int rr = 0; rr < lim; rr++) {
                d_cf_stream(s, sp, __shfl(sA, rr), __shfl(eA, rr), me, lane);
                d_cf_stream(s, sp, __shfl(sB, rr), __shfl(eB, rr), me, lane);
            }
        }
        if (c0 - R <= 0 && c0 + R >= P.g[0] - 1 && c1 - R <= 0 && c1 + R >= P.g[1] - 1 && c2 - R <= 0 && c2 + R >= P.g[2] - 1) { done = true; break; }      // every finite point seen
        if (s.cnt >= k1) {
            if (s.cnt > k1 || !s.haveT) d_cf_reduce(s, lane);
            double bound = 0.0;
            if (R > 0) { const double e = (double)P.h * ((double)R - 1.0 / 64.0); bound = e * e * (1.0 - 1.0 / 1048576.0); }
            if ((double)s.T <= bound) done = true;
        }
    }
    if (!done) { if (lane == 0) a.list[(size_t)b * a.np + atomicAdd(&a.listN[b], 1)] = q; return; }
    const float d = d_cf_finish(s, lane);
    if (lane == 0) a.dist[(size_t)b * a.np + __float_as_int(me.w)] = d;
}

__global__ __launch_bounds__(64) void k_cf_brute(CfArrays a, int k1) {
    __shared__ __align__(16) float buf[CF_CAP];
    const int b = blockIdx.y, lane = threadIdx.x;
    if ((int)blockIdx.x >= a.listN[b]) return;
    const CfPlan P = a.plan[b];
    const float4* sp = a.sorted + (size_t)b * a.np;
    const float4 me = sp[a.list[(size_t)b * a.np + blockIdx.x]];
    CfSel s{buf, 0, 0.0f, false, k1};
    d_cf_stream(s, sp, 0, P.nf, me, lane);
    const float d = d_cf_finish(s, lane);
    if (lane == 0) a.dist[(size_t)b * a.np + __float_as_int(me.w)] = d;
}

__global__ __launch_bounds__(1024) void k_cf_stats(CfArrays a, double stddevMul, int nchunks) {
    __shared__ float stage[CF_CHUNK]; __shared__ double thr;
    const int b = blockIdx.x, t = threadIdx.x, n = a.n[b];
    const CfPlan P = a.plan[b];
    const float* dist = a.dist + (size_t)b * a.np;
    CfAcc acc;
    if (!P.degenerate)
        for (int c = 0; c < n; c += CF_CHUNK) {
            stage[t] = c + t < n ? dist[c + t] : 0.0f;
            __syncthreads();
            if (t == 0) { const int m = min(CF_CHUNK, n - c); for (int i = 0; i < m; i++) acc.add(stage[i]); }      // the contract's chain, in index order
            __syncthreads();
        }
    if (t == 0) {
        CfStats st; st.mean = st.stddev = st.threshold = 0.0; st.valid = P.nf; st.degenerate = P.degenerate; st.nBrute = a.listN[b]; st.nRing = P.degenerate ? 0 : P.nf - st.nBrute;
        if (!P.degenerate) { const CfMoments m = cf_moments(acc, P.nf, stddevMul); st.mean = m.mean; st.stddev = m.stddev; st.threshold = m.threshold; }
        a.stats[b] = st; thr = st.threshold;
    }
    __syncthreads();
    const double threshold = thr; int running = 0;
    for (int c = 0; c < nchunks; c++) {
        const int i = c * CF_CHUNK + t;
        const int cnt = __syncthreads_count(i < n && (P.degenerate || !cf_removed(dist[i], threshold)));
        if (t == 0) a.chunkOff[(size_t)b * nchunks + c] = running;
        running += cnt;
    }
    if (t == 0) a.nOut[b] = running;
}

__global__ __launch_bounds__(CF_CHUNK) void k_cf_compact(CfArrays a, int nchunks) {
    __shared__ int wcnt[CF_CHUNK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63, n = a.n[b], i = chunk * CF_CHUNK + t;
    if (chunk * CF_CHUNK >= n) return;                                   // the whole block
    const CfStats st = a.stats[b];
    const bool keep = i < n && (st.degenerate || !cf_removed(a.dist[(size_t)b * a.np + i], st.threshold));
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wcnt[w];
    a.out[(size_t)b * a.np + a.chunkOff[(size_t)b * nchunks + chunk] + rank] = a.pts[(size_t)b * a.stride + i];
}

int launch_cloud_filter(const CfArrays& a, int B, int nmax, int mean_k, double stddev_mul, hipStream_t s) {
    const int nchunks = divup(a.np, CF_CHUNK), used = std::max(1, divup(nmax, CF_CHUNK)), k1 = mean_k + 1;
    HIP_TRY(hipMemsetAsync(a.cursor, 0, (size_t)B * CF_CELLS * sizeof(int), s));
    hipLaunchKernelGGL(k_cf_init, dim3(B), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_cf_bbox, dim3(used, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cf_plan, dim3(B), dim3(64), 0, s, a, k1);
    hipLaunchKernelGGL(k_cf_count, dim3(used, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cf_scan, dim3(B), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_cf_scatter, dim3(used, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cf_search, dim3(std::max(1, nmax), B), dim3(64), 0, s, a, k1);
    hipLaunchKernelGGL(k_cf_brute, dim3(std::max(1, nmax), B), dim3(64), 0, s, a, k1);
    hipLaunchKernelGGL(k_cf_stats, dim3(B), dim3(1024), 0, s, a, stddev_mul, nchunks);
    hipLaunchKernelGGL(k_cf_compact, dim3(used, B), dim3(CF_CHUNK), 0, s, a, nchunks);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
