// Occupancy map of the mapping consumer on the device (include/sind_hip.h "sind_occmap_*"; the arithmetic is host/occmap.hpp, shared with the host twin).
//
// The table is open addressing with linear probing on the packed 48-bit key.  A slot is claimed with a 64-bit compare-and-swap and its key never changes until clear.
// Which slot a voxel gets depends on who arrives first; nothing that leaves the device depends on it.
//
// A voxel's value depends on the ORDER of its hits and misses (the clamp), and the contract's order is the point index.  A ray touches a voxel at most once, and
// all rays of a key frame share the origin, so per voxel the key frame is a sequence "misses, hit, misses, hit, ..." in which only the NUMBER of misses between two
// consecutive end points matters.  Hence, per key frame:
//   k_occ_begin            zero the gap counters, reset the key frame's counters
//   k_occ_ends (cast)      one lane per ray: claim the end voxel, count the voxel's end points
//   k_occ_alloc            one lane per touched voxel: a row of m + 1 entries for a voxel with m end points (an atomic cursor; the rows' order is invisible)
//   k_occ_scatter, k_occ_rank   the voxel's point ids into its row, then each id to the position of its rank: the row sorted, with no sort
//   k_occ_dda              one lane per ray walks computeRayKeys once; per traversed voxel claim or find the slot, then add 1 to an INTEGER counter: the voxel's miss
//                          counter if no point ends there, else the counter of the gap that the ray's id falls in (binary search in the sorted row)
//   k_occ_ends (colour)    the finite points that cast no ray (z < 0, or an origin outside the keys) only colour: they LOOK UP their voxel (no claim: an unknown
//                          voxel stays out of the table) and join it if it is known or was touched by this key frame's rays.  A voxel cannot hold both kinds of point:
//                          z >= 0 and z < 0 never share a z key, and with an invalid origin no ray is cast at all.  So the per-slot fields serve both rounds.
//   k_occ_alloc, k_occ_scatter, k_occ_rank   again, for those voxels; this k_occ_alloc also counts the voxels that the key frame makes known
//   k_occ_replay           one lane per touched voxel: gap-0 misses, hit, gap-1 misses, hit, ... (a run of n equal updates stops when the value stops changing, so the
//                          camera's own voxel costs nothing special), then the colour blends in id order; resets the per-slot fields it used.
// All cross-lane accumulation is integer atomics: no floating-point atomic and no unordered floating-point sum decides a value.
// Capacity: known-before + newly-known > max_voxels, or more than `limit` claimed slots, sets the overflow flag; from then on every kernel of the call only cleans up
// (the replay resets the fields and writes no value), which is the unchanged-map guarantee.  The host reads the flag in the call's one wait.
#include "occmap_dev.hpp"

namespace sind {

namespace {

constexpr int OCC_TOUCH_BLOCKS = 1024;

__device__ __forceinline__ void occ_fail(const OccArrays& a, int b) { atomicMin(&a.ctl[OCC_FAILED], b); a.ctl[OCC_OVERFLOW] = 1; }
__device__ __forceinline__ bool occ_failed(const OccArrays& a) { return __atomic_load_n(&a.ctl[OCC_OVERFLOW], __ATOMIC_RELAXED) != 0; }

// the slot of k, claimed if absent; -1 after an overflow.  At most S probes whatever happens.
__device__ int occ_claim(const OccArrays& a, unsigned long long k, int b) {
    unsigned h = occ_hash(k) & (unsigned)(a.S - 1);
    for (int probe = 0; probe < a.S; probe++, h = (h + 1) & (unsigned)(a.S - 1)) {
        unsigned long long cur = __atomic_load_n(&a.slot[h].key, __ATOMIC_RELAXED);
        if (cur == OCC_EMPTY) {
            if (occ_failed(a)) return -1;
            cur = atomicCAS(&a.slot[h].key, (unsigned long long)OCC_EMPTY, k);
            if (cur == OCC_EMPTY) {
                if (atomicAdd(&a.ctl[OCC_CLAIMED], 1) >= a.limit) { occ_fail(a, b); return -1; }     // the slot stays claimed and unknown
                return (int)h;
            }
        }
        if (cur == k) return (int)h;
    }
    occ_fail(a, b); return -1;
}
// the first toucher of a slot in key frame `gen` appends it to the touched list
__device__ __forceinline__ void occ_touch(const OccArrays& a, int slot, int gen) {
    if (__atomic_load_n(&a.slot[slot].stamp, __ATOMIC_RELAXED) == gen) return;
    if (atomicExch(&a.slot[slot].stamp, gen) != gen) a.touched[atomicAdd(&a.ctl[OCC_NTOUCHED], 1)] = slot;
}

__global__ __launch_bounds__(256) void k_occ_clear(OccArrays a) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < a.S; s += gridDim.x * 256) {
        a.slot[s].key = OCC_EMPTY; a.slot[s].val = 0.0f; a.slot[s].col = 0; a.slot[s].stamp = 0; a.slot[s].miss = 0; a.slot[s].hits = 0; a.slot[s].off = -1; a.fill[s] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < OCC_NCTL) a.ctl[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void k_occ_begin(OccArrays a, int nGap, int b) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nGap; i += gridDim.x * 256) a.gap[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (b == 0) { a.ctl[OCC_OVERFLOW] = 0; a.ctl[OCC_FAILED] = 0x7fffffff; }
        a.ctl[OCC_NTOUCHED] = 0; a.ctl[OCC_CURSOR] = 0; a.ctl[OCC_NEW] = 0; a.ctl[OCC_KNOWN_BEFORE] = a.ctl[OCC_KNOWN];
    }
}

struct OccFrame { float o[3]; int ko[3]; int originValid, gen, b; };

// colour = 0: the points that cast a ray claim their end voxel.  colour = 1: the finite points that cast none look theirs up.
__global__ __launch_bounds__(256) void k_occ_ends(OccArrays a, OccParams P, const CloudPoint* pts, int n, OccFrame f, int colour) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    a.pslot[i] = -1;
    if (occ_failed(a)) return;
    const CloudPoint p = pts[i];
    if (!occ_finite(p.x, p.y, p.z)) return;
    const bool wants = p.z >= 0.0f;                                   // :306
    int ke[3]; const bool endValid = occ_key3(P, p.x, p.y, p.z, ke);
    OccStats* st = a.stats + f.b;
    if (!colour) {
        if (!wants) return;
        if (!f.originValid || !endValid) { atomicAdd(&st->nSkipped, 1); return; }
        atomicAdd(&st->nRays, 1);
        const int slot = occ_claim(a, occ_pack(ke), f.b);
        if (slot < 0) return;
        occ_touch(a, slot, f.gen); atomicAdd(&a.slot[slot].hits, 1); a.pslot[i] = slot;
    } else {
        if ((wants && f.originValid) || !endValid) return;
        const int slot = occ_lookup(a, occ_pack(ke));
        if (slot < 0 || a.slot[slot].off >= 0) return;                      // (a row of the first round is never extended: it cannot happen, see above, and must not overrun)
        if (!(a.slot[slot].col >> 24) && __atomic_load_n(&a.slot[slot].stamp, __ATOMIC_RELAXED) != f.gen) return;      // unknown and not on any ray of this key frame
        occ_touch(a, slot, f.gen); atomicAdd(&a.slot[slot].hits, 1); a.pslot[i] = slot;
    }
}

// countNew = 1 in the second round: a touched voxel that is unknown gets an update from this key frame (a row from the first round: hits; else misses)
__global__ __launch_bounds__(256) void k_occ_alloc(OccArrays a, int countNew) {
    const int nt = a.ctl[OCC_NTOUCHED];
    for (int t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
        const int slot = a.touched[t], m = a.slot[slot].hits, o = a.slot[slot].off;
        if (m > 0 && o < 0) a.slot[slot].off = atomicAdd(&a.ctl[OCC_CURSOR], m + 1);
        if (countNew && !(a.slot[slot].col >> 24) && (o >= 0 || a.slot[slot].miss > 0)) atomicAdd(&a.ctl[OCC_NEW], 1);
    }
}

__global__ __launch_bounds__(256) void k_occ_scatter(OccArrays a, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = a.pslot[i];
    if (slot < 0) return;
    a.ids[a.slot[slot].off + atomicAdd(&a.fill[slot], 1)] = i;
}

__global__ __launch_bounds__(256) void k_occ_rank(OccArrays a, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = a.pslot[i];
    if (slot < 0) return;
    const int o = a.slot[slot].off, m = a.slot[slot].hits;
    int rank = 0;
    for (int j = 0; j < m; j++) rank += a.ids[o + j] < i;
    a.sorted[o + rank] = i;
}

// one miss of ray i on the voxel with key k; false after an overflow
__device__ __forceinline__ bool occ_miss(const OccArrays& a, unsigned long long k, int i, const OccFrame& f) {
    const int slot = occ_claim(a, k, f.b);
    if (slot < 0) return false;
    occ_touch(a, slot, f.gen);
    const int m = a.slot[slot].hits;
    if (m == 0) { atomicAdd(&a.slot[slot].miss, 1); return true; }
    const int o = a.slot[slot].off;
    int lo = 0, hi = m;                                               // the number of the voxel's end points with an id below i
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.sorted[o + mid] < i) lo = mid + 1; else hi = mid; }
    atomicAdd(&a.gap[o + lo], 1);
    return true;
}

__global__ __launch_bounds__(64) void k_occ_dda(OccArrays a, OccParams P, const CloudPoint* pts, int n, OccFrame f) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || !f.originValid || occ_failed(a)) return;
    const CloudPoint p = pts[i];
    if (!occ_finite(p.x, p.y, p.z) || !(p.z >= 0.0f)) return;
    const float e[3] = {p.x, p.y, p.z};
    int ke[3];
    if (!occ_key3(P, p.x, p.y, p.z, ke)) return;
    if (ke[0] == f.ko[0] && ke[1] == f.ko[1] && ke[2] == f.ko[2]) return;
    OccRay r; occ_ray_init(P, f.o, e, f.ko, ke, r);
    int misses = 0;
    if (occ_miss(a, occ_pack(f.ko), i, f)) {
        misses = 1;
        while (occ_ray_step(r)) { if (!occ_miss(a, occ_pack(r.k0, r.k1, r.k2), i, f)) break; misses++; }
    }
    atomicAdd(&a.stats[f.b].nMissUpdates, misses);
}

__global__ __launch_bounds__(256) void k_occ_replay(OccArrays a, OccParams P, const CloudPoint* pts, OccFrame f) {
    const int nt = a.ctl[OCC_NTOUCHED];
    const bool over = a.ctl[OCC_OVERFLOW] != 0 || a.ctl[OCC_KNOWN_BEFORE] + a.ctl[OCC_NEW] > a.maxVoxels;      // the same verdict in every lane
    OccStats* st = a.stats + f.b;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
        const int slot = a.touched[t], m = a.slot[slot].hits, o = a.slot[slot].off, nm = a.slot[slot].miss;
        a.slot[slot].miss = 0; a.slot[slot].hits = 0; a.slot[slot].off = -1; a.fill[slot] = 0;
        if (over) continue;
        const uint32_t c = a.slot[slot].col;
        OccVoxel x; x.v = a.slot[slot].val; x.r = c & 255; x.g = (c >> 8) & 255; x.b = (c >> 16) & 255; x.known = c >> 24;
        const bool wasKnown = x.known;
        occ_update_run(P, x, P.missLog, nm);
        for (int j = 0; j < m; j++) {
            occ_update_run(P, x, P.missLog, a.gap[o + j]);
            if (f.originValid && pts[a.sorted[o + j]].z >= 0.0f) occ_update(P, x, P.hitLog);
        }
        if (m > 0) occ_update_run(P, x, P.missLog, a.gap[o + m]);
        if (x.known && m > 0) {
            const double prob = occ_probability(x.v);
            for (int j = 0; j < m; j++) { const CloudPoint p = pts[a.sorted[o + j]]; occ_colour(x, p.r, p.g, p.b, prob); }
            atomicAdd(&st->nColoured, m);
        }
        if (x.known) { a.slot[slot].val = x.v; a.slot[slot].col = (uint32_t)x.r | ((uint32_t)x.g << 8) | ((uint32_t)x.b << 16) | (1u << 24); }
        if (x.known && !wasKnown) { atomicAdd(&a.ctl[OCC_KNOWN], 1); atomicAdd(&st->nNewVoxels, 1); }
    }
    if (over && blockIdx.x == 0 && threadIdx.x == 0) occ_fail(a, f.b);
}

__global__ __launch_bounds__(256) void k_occ_occupied(OccArrays a, float occLog, unsigned long long* outKey, uint32_t* outCol, int cap, int* counter) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < a.S; s += gridDim.x * 256) {
        const unsigned long long k = a.slot[s].key; const uint32_t c = a.slot[s].col;
        if (k == OCC_EMPTY || !(c >> 24) || !(a.slot[s].val >= occLog)) continue;
        const int pos = atomicAdd(counter, 1);
        if (pos < cap) { outKey[pos] = k; outCol[pos] = c; }
    }
}

__global__ __launch_bounds__(256) void k_occ_read(OccArrays a, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = occ_lookup(a, occ_pack(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]));
    const uint32_t c = slot >= 0 ? a.slot[slot].col : 0; const bool k = (c >> 24) != 0;
    known[i] = k; logodds[i] = k ? __float_as_uint(a.slot[slot].val) : 0u;
    rgb[3 * i] = k ? (c & 255) : 0; rgb[3 * i + 1] = k ? ((c >> 8) & 255) : 0; rgb[3 * i + 2] = k ? ((c >> 16) & 255) : 0;
}

int slot_blocks(const OccArrays& a) { return std::max(1, std::min(divup(a.S, 256), 4096)); }

}  // namespace

int launch_occmap_clear(const OccArrays& a, hipStream_t s) {
    hipLaunchKernelGGL(k_occ_clear, dim3(slot_blocks(a)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_occmap_keyframe(const OccArrays& a, const OccParams& P, const CloudPoint* pts, int n, const float origin[3], int gen, int b, hipStream_t s) {
    OccFrame f{}; f.gen = gen; f.b = b;
    for (int i = 0; i < 3; i++) f.o[i] = origin[i];
    f.originValid = occ_key3(P, origin[0], origin[1], origin[2], f.ko);
    const int blocks = std::max(1, divup(n, 256));
    hipLaunchKernelGGL(k_occ_begin, dim3(blocks), dim3(256), 0, s, a, 2 * n, b);
    hipLaunchKernelGGL(k_occ_ends, dim3(blocks), dim3(256), 0, s, a, P, pts, n, f, 0);
    hipLaunchKernelGGL(k_occ_alloc, dim3(OCC_TOUCH_BLOCKS), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_occ_scatter, dim3(blocks), dim3(256), 0, s, a, n);
    hipLaunchKernelGGL(k_occ_rank, dim3(blocks), dim3(256), 0, s, a, n);
    hipLaunchKernelGGL(k_occ_dda, dim3(std::max(1, divup(n, 64))), dim3(64), 0, s, a, P, pts, n, f);
    hipLaunchKernelGGL(k_occ_ends, dim3(blocks), dim3(256), 0, s, a, P, pts, n, f, 1);
    hipLaunchKernelGGL(k_occ_alloc, dim3(OCC_TOUCH_BLOCKS), dim3(256), 0, s, a, 1);
    hipLaunchKernelGGL(k_occ_scatter, dim3(blocks), dim3(256), 0, s, a, n);
    hipLaunchKernelGGL(k_occ_rank, dim3(blocks), dim3(256), 0, s, a, n);
    hipLaunchKernelGGL(k_occ_replay, dim3(OCC_TOUCH_BLOCKS), dim3(256), 0, s, a, P, pts, f);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_occmap_occupied(const OccArrays& a, float occLog, unsigned long long* outKey, uint32_t* outCol, int cap, int* counter, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(counter, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_occ_occupied, dim3(slot_blocks(a)), dim3(256), 0, s, a, occLog, outKey, outCol, cap, counter);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_occmap_read(const OccArrays& a, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb, hipStream_t s) {
    hipLaunchKernelGGL(k_occ_read, dim3(std::max(1, divup(n, 256))), dim3(256), 0, s, a, keys, n, known, logodds, rgb);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
