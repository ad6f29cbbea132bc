// Device-resident occupancy map interface (include/sind_hip.h "sind_occmap_*"); kernels in occmap_kernels.hip, the arithmetic in host/occmap.hpp.
#pragma once
#include "common.hpp"
#include "cloud.hpp"
#include "host/occmap.hpp"
#include "host/occmap_tree.hpp"

namespace sind {

struct OccStats { int nRays, nSkipped, nColoured, nMissUpdates, nNewVoxels; };     // = sind_occmap_stats
enum { OCC_OVERFLOW = 0, OCC_CLAIMED, OCC_KNOWN, OCC_KNOWN_BEFORE, OCC_NTOUCHED, OCC_CURSOR, OCC_NEW, OCC_FAILED, OCC_NCTL };
constexpr int OCC_LAUNCHES_PER_KEYFRAME = 11;

// One slot of the table, 32 bytes: what a step of a ray needs (key, stamp, hits, miss or off) lies in one cache line, and so do the next slots of the probe.
struct OccSlot {
    unsigned long long key;                  // packed key, OCC_EMPTY when free; claimed with a 64-bit compare-and-swap, never changed until clear
    int stamp;                               // serial number of the last key frame that touched the slot
    int hits;                                // points of this key frame that end in the voxel                } zero / -1 between key frames:
    int miss;                                // misses of this key frame on a voxel with no end point in it   } the replay resets what it used
    int off;                                 // the voxel's row in ids / sorted / gap, -1 without one          }
    float val;                               // log-odds
    uint32_t col;                            // r | g << 8 | b << 16 | known << 24
};
static_assert(sizeof(OccSlot) == 32, "a slot is 32 bytes");

struct OccArrays {                           // device pointers; S = slots (a power of two), np = max_points
    int S, limit, maxVoxels;                 // a claim beyond `limit` slots is an overflow, so the table never fills and every probe ends
    OccSlot* slot;                           // [S]
    int* fill;                               // [S]  scatter cursor, zero between key frames
    int* touched;                            // [S]  slots touched by this key frame
    int* pslot;                              // [np] the slot a point ends in during the current list round, -1 if it is not in it
    int* ids; int* sorted; int* gap;         // [2 np]  per voxel with m end points a row of m + 1: ids in arrival order, in ascending order, and misses per gap
    int* ctl;                                // [OCC_NCTL]
    OccStats* stats;                         // [B]
};

#if defined(__HIPCC__)
// the hash of both tables (the flat map's and the snapshot tree's) and the flat map's lookup, shared by occmap_kernels.hip and occmap_tree.hip
__device__ __forceinline__ unsigned occ_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k;
}
__device__ inline int occ_lookup(const OccArrays& a, unsigned long long k) {
    unsigned h = occ_hash(k) & (unsigned)(a.S - 1);
    for (int probe = 0; probe < a.S; probe++, h = (h + 1) & (unsigned)(a.S - 1)) {
        const unsigned long long cur = a.slot[h].key;
        if (cur == k) return (int)h;
        if (cur == OCC_EMPTY) return -1;
    }
    return -1;
}
#endif

int launch_occmap_clear(const OccArrays& a, hipStream_t s);
// one key frame: OCC_LAUNCHES_PER_KEYFRAME launches whatever the cloud; b is the key frame's index in the call (b == 0 also resets the call's overflow state)
int launch_occmap_keyframe(const OccArrays& a, const OccParams& P, const CloudPoint* pts, int n, const float origin[3], int gen, int b, hipStream_t s);
int launch_occmap_occupied(const OccArrays& a, float occLog, unsigned long long* outKey, uint32_t* outCol, int cap, int* counter, hipStream_t s);
int launch_occmap_read(const OccArrays& a, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb, hipStream_t s);

// ---- the snapshot tree (occmap_tree.hip): inner nodes in one hash table named by (depth, key prefix), built bottom-up from the flat table, read top-down
// One node, 64 bytes.  Until its level is finalised a node only RECEIVES integer atomics from its children; the finalising lane then writes val / col / cnt.
struct OccTreeNode {
    unsigned long long name;                 // occ_tree_name, OCC_EMPTY when free; claimed with a 64-bit compare-and-swap
    unsigned long long lo, hi;               // minimum and maximum of the children's occ_tree_item: equal iff all are equal; hi's upper half is the maximum value
    unsigned long long colSum;               // occ_tree_colour_term of the children, summed
    unsigned long long cnt;                  // nodes | leaves << 32 of the subtree: the children's sum, after finalising with the node itself
    unsigned int kids;                       // child mask | number of children without children << 8
    int nOcc;                                // occupied leaves of the subtree
    float val; uint32_t col;                 // after finalising: value, colour | leaf << 24
    int idx, leafIdx;                        // top-down: the node's place in pre-order (-1: dead or not reached) and the number of listed leaves before its subtree
};
static_assert(sizeof(OccTreeNode) == 64, "a node is 64 bytes");

enum { OCCT_OVERFLOW = 0, OCCT_NNODES, OCCT_NLEAVES, OCCT_NOCC, OCCT_LEVEL, OCCT_COLLAPSED = OCCT_LEVEL + 16, OCCT_NCTL = OCCT_COLLAPSED + 16 };
constexpr int OCC_TREE_LAUNCHES_UP = 18, OCC_TREE_LAUNCHES_DOWN = 16;

struct OccTreeArrays {
    int T, maxInner;                         // slots (a power of two, at least 2 maxInner) and the most inner nodes a tree may have
    OccTreeNode* node;                       // [T]
    int* list;                               // [maxInner] slots in claim order: level 15 first, then 14, ...; a level is claimed by ONE kernel, so it is one contiguous run
    int* ctl;                                // [OCCT_NCTL]; OCCT_LEVEL + d: inner nodes of depth d; OCCT_COLLAPSED + d: nodes of depth d that pruneNode collapsed
};
struct OccTreeOut { unsigned long long* data; int capNodes; CloudPoint* leaves; uint8_t* depth; int capLeaves; };

// clear, the voxels into depth 15, then one kernel per depth 15 .. 0: OCC_TREE_LAUNCHES_UP launches whatever the map
int launch_occmap_tree_up(const OccArrays& a, const OccTreeArrays& t, const OccParams& P, int prune, int innerColour, hipStream_t s);
// one kernel per depth 0 .. 15: OCC_TREE_LAUNCHES_DOWN launches
int launch_occmap_tree_down(const OccArrays& a, const OccTreeArrays& t, const OccParams& P, int occupiedOnly, const OccTreeOut& o, hipStream_t s);

}  // namespace sind
