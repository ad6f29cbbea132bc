// Host twin of sind_occmap_* (include/sind_hip.h): the literal sequential loops of the contract over a flat unordered_map, with the arithmetic of occmap.hpp and
// nothing of the device's scheduling.  Per key frame: every ray in point order (the miss list in order, then the hit), then every colour in point order.
// SIND_E_CAPACITY must leave the map as it was: a key frame first walks its rays without writing and counts the voxels it would make known.
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "occmap_twin.hpp"
#include "sind_hip.h"

using namespace sind;

namespace {

bool params_ok(double res, const double p[5], int maxVoxels, int maxPoints) {
    if (!(res >= SIND_OCCMAP_MIN_RESOLUTION && res <= SIND_OCCMAP_MAX_RESOLUTION) || maxVoxels < 1 || maxPoints < 1) return false;
    for (int i = 0; i < 5; i++) if (!(p[i] > 0.0 && p[i] < 1.0)) return false;
    return p[2] < p[3];
}

// the ray of one point: fn(packed key, is_hit) for every key of the miss list in order, then for the end key.  Returns false if the ray is skipped.
template <class F> bool walk_ray(const OccParams& P, const float o[3], const float e[3], F fn) {
    int ko[3], ke[3];
    if (!occ_key3(P, o[0], o[1], o[2], ko) || !occ_key3(P, e[0], e[1], e[2], ke)) return false;
    if (ko[0] != ke[0] || ko[1] != ke[1] || ko[2] != ke[2]) {
        OccRay r; occ_ray_init(P, o, e, ko, ke, r);
        fn(occ_pack(ko), false);
        while (occ_ray_step(r)) fn(occ_pack(r.k0, r.k1, r.k2), false);
    }
    fn(occ_pack(ke), true);
    return true;
}

int insert_one(sindh_occmap* h, const sind_cloud_point* p, int n, const float* origin, sind_occmap_stats* st) {
    const OccParams& P = h->P; sind_occmap_stats s{};
    if (!occ_finite(origin[0], origin[1], origin[2])) return SIND_E_ARG;
    std::unordered_set<uint64_t> fresh;
    for (int i = 0; i < n; i++) {
        if (!occ_finite(p[i].x, p[i].y, p[i].z) || !(p[i].z >= 0.0f)) continue;
        const float e[3] = {p[i].x, p[i].y, p[i].z};
        walk_ray(P, origin, e, [&](uint64_t k, bool) { auto it = h->map.find(k); if (it == h->map.end() || !it->second.known) fresh.insert(k); });
    }
    if (h->map.size() + fresh.size() > (size_t)h->maxVoxels) return SIND_E_CAPACITY;
    s.n_new_voxels = (int)fresh.size();
    for (int i = 0; i < n; i++) {
        if (!occ_finite(p[i].x, p[i].y, p[i].z) || !(p[i].z >= 0.0f)) continue;
        const float e[3] = {p[i].x, p[i].y, p[i].z};
        const bool cast = walk_ray(P, origin, e, [&](uint64_t k, bool hit) { occ_update(P, h->map[k], hit ? P.hitLog : P.missLog); if (!hit) s.n_miss_updates++; });
        if (cast) s.n_rays++; else s.n_skipped++;
    }
    for (int i = 0; i < n; i++) {
        if (!occ_finite(p[i].x, p[i].y, p[i].z)) continue;
        int k[3];
        if (!occ_key3(P, p[i].x, p[i].y, p[i].z, k)) continue;
        auto it = h->map.find(occ_pack(k));
        if (it == h->map.end() || !it->second.known) continue;
        occ_colour(it->second, p[i].r, p[i].g, p[i].b, occ_probability(it->second.v)); s.n_coloured++;
    }
    if (st) *st = s;
    return SIND_OK;
}

}  // namespace

extern "C" {

int sindh_occmap_create(double resolution, double prob_hit, double prob_miss, double clamp_min, double clamp_max, double occ_thres, int max_voxels, int max_points,
                        sindh_occmap** out) {
    const double p[5] = {prob_hit, prob_miss, clamp_min, clamp_max, occ_thres};
    if (!out || !params_ok(resolution, p, max_voxels, max_points)) return SIND_E_ARG;
    sindh_occmap* h = new sindh_occmap(); h->P = occ_params(resolution, p[0], p[1], p[2], p[3], p[4]); h->maxVoxels = max_voxels; h->maxPoints = max_points;
    *out = h; return SIND_OK;
}
int sindh_occmap_destroy(sindh_occmap* h) { delete h; return SIND_OK; }
int sindh_occmap_clear(sindh_occmap* h) { if (!h) return SIND_E_ARG; h->map.clear(); return SIND_OK; }
int sindh_occmap_size(sindh_occmap* h) { return h ? (int)h->map.size() : SIND_E_ARG; }

int sindh_occmap_insert(sindh_occmap* h, int B, const sind_cloud_point* points, int stride, const int* n_points, const float* origins, sind_occmap_stats* stats) {
    if (!h || B < 0 || (B > 0 && (!n_points || !origins)) || stride < 0) return SIND_E_ARG;
    for (int b = 0; b < B; b++) {
        if (n_points[b] < 0 || n_points[b] > stride || (n_points[b] > 0 && !points) || !occ_finite(origins[3 * b], origins[3 * b + 1], origins[3 * b + 2])) return SIND_E_ARG;
        if (n_points[b] > h->maxPoints) return SIND_E_CAPACITY;
    }
    if (stats && B) std::memset(stats, 0, (size_t)B * sizeof(sind_occmap_stats));
    for (int b = 0; b < B; b++) {
        const int rc = insert_one(h, points ? points + (size_t)b * stride : nullptr, n_points[b], origins + 3 * b, stats ? stats + b : nullptr);
        if (rc != SIND_OK) return rc;                                 // as B calls in order: the key frames before b are in the map, b and the later ones are not
    }
    return SIND_OK;
}

int sindh_occmap_occupied(sindh_occmap* h, sind_cloud_point* out, int cap, int* n_out) {
    if (!h || !n_out || (out && cap < 0)) return SIND_E_ARG;
    std::vector<std::pair<uint64_t, uint64_t>> v;
    for (const auto& kv : h->map) if (kv.second.known && kv.second.v >= h->P.occLog) v.emplace_back(occ_morton(kv.first), kv.first);
    std::sort(v.begin(), v.end());
    *n_out = (int)v.size();
    if (!out) return SIND_OK;
    if ((int)v.size() > cap) return SIND_E_CAPACITY;
    for (size_t i = 0; i < v.size(); i++) {
        const uint64_t k = v[i].second; const OccVoxel& x = h->map[k];
        out[i].x = (float)occ_coord(h->P, (int)(k & 0xffff)); out[i].y = (float)occ_coord(h->P, (int)((k >> 16) & 0xffff)); out[i].z = (float)occ_coord(h->P, (int)((k >> 32) & 0xffff));
        out[i].b = x.b; out[i].g = x.g; out[i].r = x.r; out[i].a = 0;
    }
    return SIND_OK;
}

int sindh_occmap_read(sindh_occmap* h, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb) {
    if (!h || n < 0 || (n > 0 && (!keys || !known || !logodds || !rgb))) return SIND_E_ARG;
    for (int i = 0; i < n; i++) {
        auto it = h->map.find(occ_pack(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]));
        const bool k = it != h->map.end() && it->second.known;
        known[i] = k; logodds[i] = 0; rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0;
        if (k) { std::memcpy(logodds + i, &it->second.v, 4); rgb[3 * i] = it->second.r; rgb[3 * i + 1] = it->second.g; rgb[3 * i + 2] = it->second.b; }
    }
    return SIND_OK;
}

}  // extern "C"
