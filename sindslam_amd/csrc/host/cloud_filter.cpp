// Host twin of sind_cloud_filter_outliers (include/sind_hip.h): the arithmetic of cloud_filter.hpp over an exact search of its own.
// Search: a uniform grid over the bounding box of the finite points, the cell index of a coordinate being a MONOTONE function of it (FP32 subtract, multiply,
// truncate, clamp are all monotone).  Per axis and cell index the grid keeps lo[i] = the smallest coordinate among the points with index >= i and hi[i] = the
// largest among those with index <= i.  A point outside the box of Chebyshev radius R around the query's cell has, on some axis, an index above c + R or below
// c - R, hence a coordinate >= lo[c + R + 1] >= q or <= hi[c - R - 1] <= q; FP32 subtraction and squaring are monotone in |q - x|, and d = fl(fl(dx*dx) + ..) only
// grows when non-negative terms are added, so fl(fl(q - edge)^2) bounds the contract's squared distance from below IN FP32, with no rounding analysis at all.
// The search stops at the first R whose (mean_k + 1)-th smallest candidate is <= that bound (a point at exactly the bound cannot change the multiset).
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>
#include "cloud_filter.hpp"
#include "sind_hip.h"

namespace {

using namespace sind;

struct Grid {
    float o[3], inv[3]; int g[3];
    std::vector<float> lo[3], hi[3]; std::vector<int> start, order;
    int cell(int a, float v) const { const float t = (v - o[a]) * inv[a]; int i = t >= 0.0f ? (t < (float)g[a] ? (int)t : g[a] - 1) : 0; return i; }
};

void filter_one(const sind_cloud_point* p, int n, int k, double mul, sind_cloud_point* out, int outCap, int* nOut, float* dist, sind_cloud_filter_stats* st) {
    const float INF = std::numeric_limits<float>::infinity();
    std::vector<int> fin; fin.reserve(n);
    for (int i = 0; i < n; i++) if (cf_finite(p[i].x, p[i].y, p[i].z)) fin.push_back(i);
    const int nf = (int)fin.size(), k1 = k + 1;
    std::vector<float> d(n, 0.0f);
    sind_cloud_filter_stats s{}; s.valid = nf;
    if (nf < k1) s.degenerate = 1;
    else {
        Grid G; float mn[3] = {INF, INF, INF}, mx[3] = {-INF, -INF, -INF};
        auto co = [&](int i, int a) { return a == 0 ? p[i].x : a == 1 ? p[i].y : p[i].z; };
        for (int i : fin) for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], co(i, a)); mx[a] = std::max(mx[a], co(i, a)); }
        // about two points per cell of the occupied extent, at most 48 cells per axis; any choice is correct, the bound above comes from the data
        double ext[3], vol = 1.0; int dims = 0;
        for (int a = 0; a < 3; a++) { ext[a] = (double)mx[a] - (double)mn[a]; if (ext[a] > 0 && std::isfinite(ext[a])) { vol *= ext[a]; dims++; } }
        double h = dims ? std::pow(vol * 2.0 / nf, 1.0 / dims) : 1.0;
        for (int a = 0; a < 3; a++) if (ext[a] > 0 && std::isfinite(ext[a])) h = std::max(h, ext[a] / 47.5);
        for (int a = 0; a < 3; a++) {
            const bool flat = !(ext[a] > 0) || !std::isfinite(ext[a]) || !(h > 1e-30);
            G.o[a] = mn[a]; G.g[a] = flat ? 1 : std::min(48, (int)(ext[a] / h) + 1); G.inv[a] = flat ? 0.0f : (float)(1.0 / h);
            if (!std::isfinite(G.inv[a])) { G.inv[a] = 0.0f; G.g[a] = 1; }
        }
        const int cells = G.g[0] * G.g[1] * G.g[2];
        std::vector<int> key(nf); G.start.assign(cells + 1, 0); G.order.resize(nf);
        for (int a = 0; a < 3; a++) { G.lo[a].assign(G.g[a] + 1, INF); G.hi[a].assign(G.g[a] + 1, -INF); }
        for (int q = 0; q < nf; q++) {
            int c[3]; for (int a = 0; a < 3; a++) { const float v = co(fin[q], a); c[a] = G.cell(a, v); G.lo[a][c[a]] = std::min(G.lo[a][c[a]], v); G.hi[a][c[a]] = std::max(G.hi[a][c[a]], v); }
            key[q] = (c[2] * G.g[1] + c[1]) * G.g[0] + c[0]; G.start[key[q] + 1]++;
        }
        for (int a = 0; a < 3; a++) {
            for (int i = G.g[a] - 2; i >= 0; i--) G.lo[a][i] = std::min(G.lo[a][i], G.lo[a][i + 1]);      // suffix minimum
            for (int i = 1; i < G.g[a]; i++) G.hi[a][i] = std::max(G.hi[a][i], G.hi[a][i - 1]);           // prefix maximum
        }
        for (int c = 0; c < cells; c++) G.start[c + 1] += G.start[c];
        { std::vector<int> cur(G.start.begin(), G.start.end() - 1); for (int q = 0; q < nf; q++) G.order[cur[key[q]]++] = fin[q]; }
        std::vector<float> cand; cand.reserve(4096);
        for (int q = 0; q < nf; q++) {
            const int i = fin[q]; const float qc[3] = {p[i].x, p[i].y, p[i].z};
            int c[3]; for (int a = 0; a < 3; a++) c[a] = G.cell(a, qc[a]);
            cand.clear(); float T = INF; bool haveT = false;
            for (int R = 0;; R++) {
                for (int z = std::max(c[2] - R, 0); z <= std::min(c[2] + R, G.g[2] - 1); z++)
                    for (int y = std::max(c[1] - R, 0); y <= std::min(c[1] + R, G.g[1] - 1); y++) {
                        auto visit = [&](int x) {
                            if (x < 0 || x >= G.g[0]) return;
                            const int cellKey = (z * G.g[1] + y) * G.g[0] + x;
                            for (int r = G.start[cellKey]; r < G.start[cellKey + 1]; r++) {
                                const int j = G.order[r]; const float dd = cf_dist2(qc[0], qc[1], qc[2], p[j].x, p[j].y, p[j].z);
                                if (!haveT || dd < T) cand.push_back(dd);
                            }
                        };
                        if (std::abs(z - c[2]) == R || std::abs(y - c[1]) == R) for (int x = c[0] - R; x <= c[0] + R; x++) visit(x);      // a face of the shell
                        else { visit(c[0] - R); visit(c[0] + R); }                                                                       // R > 0 here
                    }
                if ((int)cand.size() >= k1) {
                    std::nth_element(cand.begin(), cand.begin() + k, cand.end()); cand.resize(k1); T = cand[k]; haveT = true;
                }
                float bound = INF;
                for (int a = 0; a < 3; a++) {
                    if (c[a] + R + 1 < G.g[a] && G.lo[a][c[a] + R + 1] < INF) { const float e = qc[a] - G.lo[a][c[a] + R + 1]; bound = std::min(bound, e * e); }
                    if (c[a] - R - 1 >= 0 && G.hi[a][c[a] - R - 1] > -INF) { const float e = qc[a] - G.hi[a][c[a] - R - 1]; bound = std::min(bound, e * e); }
                }
                if (haveT && T <= bound) break;
            }
            std::sort(cand.begin(), cand.end());
            d[i] = cf_mean_distance([&](int t) { return cf_root(cand[t + 1]); }, k);
        }
        CfAcc acc; for (int i = 0; i < n; i++) acc.add(d[i]);
        const CfMoments m = cf_moments(acc, nf, mul); s.mean = m.mean; s.stddev = m.stddev; s.threshold = m.threshold;
    }
    int w = 0;
    for (int i = 0; i < n; i++) if (s.degenerate || !cf_removed(d[i], s.threshold)) { if (out && w < outCap) out[w] = p[i]; w++; }
    *nOut = w;
    if (dist && n) std::memcpy(dist, d.data(), (size_t)n * sizeof(float));
    if (st) *st = s;
}

}  // namespace

extern "C" int sindh_cloud_filter_outliers(int B, const sind_cloud_point* points, int stride, const int* n_points, int mean_k, double stddev_mul, sind_cloud_point* out,
                                           int out_cap, int* n_out, float* distances, sind_cloud_filter_stats* stats) {
    if (B < 0 || !n_out || (B > 0 && !n_points) || mean_k < 1 || mean_k > sind::CF_MAX_MEAN_K || !std::isfinite(stddev_mul) || stride < 0 || (out && out_cap < 0)) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (n_points[b] < 0 || n_points[b] > stride || (n_points[b] > 0 && !points)) return SIND_E_ARG;
    int rc = SIND_OK;
    for (int b = 0; b < B; b++) {
        filter_one(points + (size_t)b * stride, n_points[b], mean_k, stddev_mul, out ? out + (size_t)b * out_cap : nullptr, out_cap, n_out + b,
                   distances ? distances + (size_t)b * stride : nullptr, stats ? stats + b : nullptr);
        if (out && n_out[b] > out_cap) rc = SIND_E_CAPACITY;
    }
    return rc;
}
