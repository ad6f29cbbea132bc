// Device-resident occupancy map interface (include/sind_hip.h "sind_occmap_*"); kernels in occmap_kernels.hip, the arithmetic in host/occmap.hpp.
#pragma once
#include "common.hpp"
#include "cloud.hpp"
#include "host/occmap.hpp"

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

int launch_occmap_clear(const OccArrays& a, hipStream_t s);
// one key frame: OCC_LAUNCHES_PER_KEYFRAME launches whatever the cloud; b is the key frame's index in the call (b == 0 also resets the call's overflow state)
int launch_occmap_keyframe(const OccArrays& a, const OccParams& P, const CloudPoint* pts, int n, const float origin[3], int gen, int b, hipStream_t s);
int launch_occmap_occupied(const OccArrays& a, float occLog, unsigned long long* outKey, uint32_t* outCol, int cap, int* counter, hipStream_t s);
int launch_occmap_read(const OccArrays& a, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb, hipStream_t s);

}  // namespace sind
