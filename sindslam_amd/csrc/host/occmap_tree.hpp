// Snapshot tree of the flat occupancy map (include/sind_hip.h, "sind_occmap_tree"): octomap's inner nodes, prune(), writeData and leaf iteration, restated from
// octomap 1.9 as recalled (OcTreeBaseImpl::prune / pruneNode / isNodeCollapsible, OccupancyOcTreeBase::updateInnerOccupancy, ColorOcTree::getAverageChildColor,
// OcTreeBaseImpl::writeData / writeNodesRecurs, AbstractOcTree::write).  Parity with a real octomap build is UNPINNED, as for the rest of the occupancy contract.
// ONE source for what the device (csrc/occmap_tree.hip) and the host twin (csrc/host/occmap_tree.cpp) must agree on: the child index, the node key and its packing,
// the order-preserving integer image of a float, the item that decides "all eight equal", the packed colour sums and their average, the 8-byte record and the leaf
// centre.  The SCHEDULE is not here: the twin builds a pointer tree and recurses, the device sweeps levels over a hash table of nodes.
#pragma once
#include <cstdio>
#include <sstream>
#include <string>
#include "occmap.hpp"

namespace sind {

constexpr int OCC_TREE_DEPTH = 16;
constexpr uint32_t OCC_WHITE = 0xffffffu;                             // r | g << 8 | b << 16 of (255, 255, 255): "not set"
constexpr uint64_t OCC_FIELDS = 0x0000000100010001ull;                // bit 0 of the x, y and z field of a packed key

// the child index at depth d of a voxel key (d = 0 .. 15): z the most significant bit, then y, then x -- the Morton order of occ_morton
SIND_HD inline int occ_tree_child(int kx, int ky, int kz, int d) { const int s = 15 - d; return (((kz >> s) & 1) << 2) | (((ky >> s) & 1) << 1) | ((kx >> s) & 1); }

// A node is (depth, prefix): depth 0 .. 16, prefix = the packed key with every field shifted right by 16 - depth.  Its 64-bit name is depth << 48 | prefix; no name
// has all bits set (depth <= 16), so OCC_EMPTY marks a free slot here too.  A depth-16 node is a voxel and its prefix is the flat map's key.
SIND_HD inline uint64_t occ_tree_prefix(uint64_t packed, int d) { return (packed >> (16 - d)) & ((uint64_t)(0xffffu >> (16 - d)) * OCC_FIELDS); }
SIND_HD inline uint64_t occ_tree_name(int d, uint64_t prefix) { return ((uint64_t)d << 48) | prefix; }
SIND_HD inline int occ_tree_name_depth(uint64_t name) { return (int)(name >> 48); }
SIND_HD inline uint64_t occ_tree_name_prefix(uint64_t name) { return name & 0xffffffffffffull; }
// a node's index among its parent's children, its parent's prefix and its child's prefix
SIND_HD inline int occ_tree_pos(uint64_t prefix) { return (int)((((prefix >> 32) & 1) << 2) | (((prefix >> 16) & 1) << 1) | (prefix & 1)); }
SIND_HD inline uint64_t occ_tree_parent(uint64_t prefix) { return (prefix >> 1) & (0x7fffull * OCC_FIELDS); }
SIND_HD inline uint64_t occ_tree_kid(uint64_t prefix, int i) { return (prefix << 1) | (uint64_t)(i & 1) | ((uint64_t)((i >> 1) & 1) << 16) | ((uint64_t)((i >> 2) & 1) << 32); }

// The order-preserving integer image of a float: a < b as floats iff image(a) < image(b) as unsigned, for every pair that holds no NaN and not both zeros of
// different sign.  Log-odds are clamped sums that start at +0: neither occurs.  An integer atomicMax over images is the float maximum, whatever the arrival order.
SIND_HD inline uint32_t occ_ord(float v) { union { float f; uint32_t u; } a; a.f = v; return a.u ^ ((a.u >> 31) ? 0xffffffffu : 0x80000000u); }
SIND_HD inline float occ_unord(uint32_t o) { union { float f; uint32_t u; } a; a.u = o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu); return a.f; }
// (value, colour) of a child in one word: eight children are equal in value (float ==) and colour iff the minimum and the maximum of their items are equal, and
// the upper half of the maximum is the image of updateOccupancyChildren's maximum
SIND_HD inline uint64_t occ_tree_item(float v, uint32_t col24) { return ((uint64_t)occ_ord(v) << 32) | col24; }
SIND_HD inline float occ_tree_item_value(uint64_t item) { return occ_unord((uint32_t)(item >> 32)); }
SIND_HD inline uint32_t occ_tree_item_colour(uint64_t item) { return (uint32_t)item & OCC_WHITE; }

// getAverageChildColor: per channel the integer sum over the existing children whose colour is set, integer-divided by their number; white if there is none.
// The sums of one node in one word (r | g << 16 | b << 32 | count << 48; a sum is at most 8 * 255), so that one integer add per child accumulates them.
SIND_HD inline uint64_t occ_tree_colour_term(uint32_t col24) {
    return col24 == OCC_WHITE ? 0ull : (uint64_t)(col24 & 255) | ((uint64_t)((col24 >> 8) & 255) << 16) | ((uint64_t)((col24 >> 16) & 255) << 32) | (1ull << 48);
}
SIND_HD inline uint32_t occ_tree_colour_average(uint64_t sums) {
    const uint32_t c = (uint32_t)(sums >> 48);
    if (!c) return OCC_WHITE;
    return ((uint32_t)(sums & 0xffff) / c) | (((uint32_t)((sums >> 16) & 0xffff) / c) << 8) | (((uint32_t)((sums >> 32) & 0xffff) / c) << 16);
}

// writeData's record of one node, 8 bytes in memory order: the FP32 value, r, g, b, then one byte with bit i set iff child i exists (0 for a leaf)
SIND_HD inline uint64_t occ_tree_record(float v, uint32_t col24, uint32_t childMask) {
    union { float f; uint32_t u; } a; a.f = v;
    return (uint64_t)a.u | ((uint64_t)(col24 & OCC_WHITE) << 32) | ((uint64_t)(childMask & 255) << 56);
}

// the centre of a leaf at depth d (1 .. 16) that holds the key k, per axis; at depth 16 it is (float) occ_coord
SIND_HD inline float occ_tree_centre(const OccParams& P, int k, int d) {
    const int s = 16 - d;
    return (float)(((double)((int)((k >> s) << s) - OCC_KEY_OFFSET) + 0.5 * (double)(1 << s)) * P.res);
}

// AbstractOcTree::write's header of an .ot file; the stream follows it.  The resolution as a default-precision ostream prints it.
inline std::string occ_tree_ot_header(int nNodes, double res) {
    std::ostringstream s;
    s << "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid ColorOcTree\nsize " << nNodes << "\nres " << res << "\ndata\n";
    return s.str();
}
// header + stream into a file; false if the file cannot be written whole
inline bool occ_tree_write_file(const char* path, const std::string& head, const uint8_t* data, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size() && (bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes);
    return std::fclose(f) == 0 && ok;
}

struct OccTreeStats { int nNodes, nInner, nLeaves, nPruned, nOccupiedLeaves; int leavesAtDepth[OCC_TREE_DEPTH + 1]; };     // = sind_occmap_tree_stats

}  // namespace sind
