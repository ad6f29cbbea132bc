// Snapshot tree of the flat occupancy map on the device (include/sind_hip.h "sind_occmap_tree"; the arithmetic is host/occmap_tree.hpp, shared with the host twin).
//
// No sort and no host work per node.  The inner nodes live in ONE hash table (open addressing, linear probing) named by (depth, key prefix); a slot is claimed with a
// 64-bit compare-and-swap, as OccSlot is.  Which slot a node gets depends on who arrives first; nothing that leaves the device depends on it.
//
// BOTTOM-UP, one kernel per level (the launches do not depend on the map):
//   k_tree_clear     every slot free, every accumulator at its identity (the table is sized from max_voxels, not from the map: a full sweep, 64 bytes per slot)
//   k_tree_voxels    one lane per slot of the FLAT table: a known voxel is a depth-16 leaf and claims its depth-15 parent.  It adds nothing: eight siblings lie in
//                    eight unrelated slots, and six atomics each on one parent took 2.5 of the call's 3.5 ms at a million voxels (profiles/occmap_tree.txt)
//   k_tree_level d   d = 15 .. 0, one lane per node of depth d: all its children have added themselves (the previous kernel; at depth 15 the lane GATHERS its up to
//                    eight voxels from the flat table instead, eight look-ups and no atomic), so it FINALISES -- collapsible iff
//                    prune, d >= 1, all eight children exist, none has children, and the minimum and the maximum of their (value image, colour) items are equal;
//                    then value, colour and subtree counts -- and adds itself to its parent of depth d - 1
//   A child adds to its parent with INTEGER atomics only: the child's bit and whether it is a leaf (one add: each child adds once, so the add is an OR), min and max of
//   the item, the packed subtree counts, the occupied leaves, the packed colour sums.  No floating-point atomic decides a value and no result depends on slot or
//   arrival order: min, max and integer sums commute.
//   PER-LEVEL NODE LISTS: a cursor at claim time.  The nodes of depth d are claimed by one kernel only (k_tree_level d + 1, or k_tree_voxels), so with one counter per
//   depth the place of a new node is (the nodes of all deeper levels, final by then) + (its ticket): every level is one contiguous run of `list`, and the kernel of
//   depth d finds its run from the counters alone.  No scan of the table per level.
//   Pruning bottom-up in one sweep equals OcTreeBaseImpl::prune()'s loop over depths on a tree that starts flat: a node of depth d can only become collapsible through
//   children that collapsed in the pass for d + 1, which is the order of both; prune()'s early break skips depths at which nothing can be collapsible any more.
// TOP-DOWN, one kernel per depth 0 .. 15, after the host has read the counts and sized the outputs:
//   k_tree_down d    one lane per node of depth d.  A node without a place (idx < 0) is dead -- its parent was pruned or is dead -- and hands nothing down.  A live
//                    node writes its own 8-byte record at 8 idx; a pruned one also its leaf record; an inner one hands each existing child its place: its own + 1 + the
//                    subtree counts of the child's earlier siblings (and likewise the number of listed leaves before it).  At depth 15 the children are voxels: the
//                    lane looks them up in the flat table and writes their records itself, so no per-voxel workspace exists.
// Capacity: more inner nodes than maxInner sets the overflow flag; claims stop, nothing is written out of bounds, and the host refuses the call.
#include "occmap_dev.hpp"

namespace sind {

namespace {

constexpr int TREE_BLOCKS = 1024;

struct TreeRun { int begin, n; };
// the run of depth d in `list`: behind the nodes of all deeper levels
__device__ __forceinline__ TreeRun tree_run(const OccTreeArrays& t, int d) {
    int begin = 0;
    for (int e = 15; e > d; e--) begin += t.ctl[OCCT_LEVEL + e];
    int n = t.ctl[OCCT_LEVEL + d];
    begin = min(begin, t.maxInner); n = min(n, t.maxInner - begin);
    return TreeRun{begin, n};
}

// the slot of the node `name` of depth d, claimed (and listed) if absent; -1 after an overflow.  At most T probes whatever happens.
__device__ int tree_claim(const OccTreeArrays& t, unsigned long long name, int d, int levelBegin) {
    unsigned h = occ_hash(name) & (unsigned)(t.T - 1);
    for (int probe = 0; probe < t.T; probe++, h = (h + 1) & (unsigned)(t.T - 1)) {
        unsigned long long cur = __atomic_load_n(&t.node[h].name, __ATOMIC_RELAXED);
        if (cur == OCC_EMPTY) {
            if (__atomic_load_n(&t.ctl[OCCT_OVERFLOW], __ATOMIC_RELAXED)) return -1;
            cur = atomicCAS(&t.node[h].name, (unsigned long long)OCC_EMPTY, name);
            if (cur == OCC_EMPTY) {
                const int pos = levelBegin + atomicAdd(&t.ctl[OCCT_LEVEL + d], 1);
                if (pos >= t.maxInner) { t.ctl[OCCT_OVERFLOW] = 1; return -1; }
                t.list[pos] = (int)h;
                return (int)h;
            }
        }
        if (cur == name) return (int)h;
    }
    t.ctl[OCCT_OVERFLOW] = 1; return -1;
}
__device__ int tree_lookup(const OccTreeArrays& t, unsigned long long name) {
    unsigned h = occ_hash(name) & (unsigned)(t.T - 1);
    for (int probe = 0; probe < t.T; probe++, h = (h + 1) & (unsigned)(t.T - 1)) {
        const unsigned long long cur = t.node[h].name;
        if (cur == name) return (int)h;
        if (cur == OCC_EMPTY) return -1;
    }
    return -1;
}

// a child (prefix at depth d + 1 of its parent's) adds itself to the parent in `slot`
__device__ __forceinline__ void tree_add(const OccTreeArrays& t, int slot, unsigned long long childPrefix, float v, uint32_t col24, bool leaf, unsigned long long cnt, int nOcc,
                                         int innerColour) {
    OccTreeNode* p = t.node + slot; const unsigned long long item = occ_tree_item(v, col24);
    atomicMin(&p->lo, item); atomicMax(&p->hi, item);
    atomicAdd(&p->kids, (1u << occ_tree_pos(childPrefix)) | (leaf ? 256u : 0u));
    atomicAdd(&p->cnt, cnt);
    if (nOcc) atomicAdd(&p->nOcc, nOcc);
    if (innerColour && col24 != OCC_WHITE) atomicAdd(&p->colSum, (unsigned long long)occ_tree_colour_term(col24));
}

__global__ __launch_bounds__(256) void k_tree_clear(OccTreeArrays t) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < t.T; s += gridDim.x * 256) {
        OccTreeNode n; n.name = OCC_EMPTY; n.lo = ~0ull; n.hi = 0; n.colSum = 0; n.cnt = 0; n.kids = 0; n.nOcc = 0; n.val = 0.0f; n.col = 0; n.idx = -1; n.leafIdx = 0;
        t.node[s] = n;
    }
    if (blockIdx.x == 0 && threadIdx.x < OCCT_NCTL) t.ctl[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void k_tree_voxels(OccArrays a, OccTreeArrays t) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < a.S; s += gridDim.x * 256) {
        const unsigned long long k = a.slot[s].key;
        if (k == OCC_EMPTY || !(a.slot[s].col >> 24)) continue;
        tree_claim(t, occ_tree_name(15, occ_tree_parent(k)), 15, 0);
    }
}

__global__ __launch_bounds__(256) void k_tree_level(OccArrays a, OccTreeArrays t, int d, int prune, int innerColour, float occLog) {
    __shared__ int sCollapsed;
    if (threadIdx.x == 0) sCollapsed = 0;
    __syncthreads();
    const TreeRun run = tree_run(t, d);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < run.n; i += gridDim.x * 256) {
        OccTreeNode* n = t.node + t.list[run.begin + i];
        const unsigned long long prefix = occ_tree_name_prefix(n->name);
        unsigned kids; unsigned long long lo, hi, cntKids, colSum; int nOccKids;
        if (d == 15) {                                                  // the children are voxels: gathered from the flat table, what tree_add would have accumulated
            kids = 0; lo = ~0ull; hi = 0; cntKids = 0; colSum = 0; nOccKids = 0;
            for (int c = 0; c < 8; c++) {
                const int slot = occ_lookup(a, occ_tree_kid(prefix, c));
                if (slot < 0 || !(a.slot[slot].col >> 24)) continue;
                const float kv = a.slot[slot].val; const uint32_t kc = a.slot[slot].col & OCC_WHITE; const unsigned long long item = occ_tree_item(kv, kc);
                kids += (1u << c) | 256u; lo = item < lo ? item : lo; hi = item > hi ? item : hi; cntKids += 1ull | (1ull << 32); nOccKids += kv >= occLog ? 1 : 0;
                colSum += occ_tree_colour_term(kc);
            }
        } else { kids = n->kids; lo = n->lo; hi = n->hi; cntKids = n->cnt; colSum = n->colSum; nOccKids = n->nOcc; }
        const unsigned mask = kids & 255u, leafKids = kids >> 8;
        const bool collapse = prune && d >= 1 && mask == 255u && leafKids == 8u && lo == hi;
        float v; uint32_t col; unsigned long long cnt; int nOcc;
        if (collapse) { v = occ_tree_item_value(lo); col = occ_tree_item_colour(lo); cnt = 1ull | (1ull << 32); nOcc = v >= occLog ? 1 : 0; atomicAdd(&sCollapsed, 1); }
        else { v = occ_tree_item_value(hi); col = innerColour ? occ_tree_colour_average(colSum) : OCC_WHITE; cnt = cntKids + 1ull; nOcc = nOccKids; }
        n->val = v; n->col = col | (collapse ? 1u << 24 : 0u); n->cnt = cnt; n->nOcc = nOcc; n->kids = kids;
        if (d == 0) {
            n->idx = 0; n->leafIdx = 0;
            t.ctl[OCCT_NNODES] = (int)(cnt & 0xffffffffull); t.ctl[OCCT_NLEAVES] = (int)(cnt >> 32); t.ctl[OCCT_NOCC] = nOcc;
        } else {
            const int slot = tree_claim(t, occ_tree_name(d - 1, occ_tree_parent(prefix)), d - 1, run.begin + run.n);
            if (slot >= 0) tree_add(t, slot, prefix, v, col, collapse, cnt, nOcc, innerColour);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && sCollapsed) atomicAdd(&t.ctl[OCCT_COLLAPSED + d], sCollapsed);
}

__device__ __forceinline__ void tree_write_leaf(const OccTreeOut& o, const OccParams& P, int at, unsigned long long prefix, int d, uint32_t col24) {
    if (!o.leaves || at < 0 || at >= o.capLeaves) return;
    const int s = 16 - d; CloudPoint p;
    p.x = occ_tree_centre(P, (int)(prefix & 0xffff) << s, d); p.y = occ_tree_centre(P, (int)((prefix >> 16) & 0xffff) << s, d); p.z = occ_tree_centre(P, (int)((prefix >> 32) & 0xffff) << s, d);
    p.r = col24 & 255; p.g = (col24 >> 8) & 255; p.b = (col24 >> 16) & 255; p.a = 0;
    o.leaves[at] = p; o.depth[at] = (uint8_t)d;
}

__global__ __launch_bounds__(256) void k_tree_down(OccArrays a, OccTreeArrays t, OccParams P, int d, int occupiedOnly, OccTreeOut o) {
    const TreeRun run = tree_run(t, d);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < run.n; i += gridDim.x * 256) {
        const OccTreeNode* n = t.node + t.list[run.begin + i];
        const int idx = n->idx;
        if (idx < 0) continue;
        const bool leaf = (n->col >> 24) != 0; const uint32_t col = n->col & OCC_WHITE, mask = n->kids & 255u; const float v = n->val;
        const unsigned long long prefix = occ_tree_name_prefix(n->name);
        if (o.data && idx < o.capNodes) o.data[idx] = occ_tree_record(v, col, leaf ? 0u : mask);
        if (leaf) {
            if (!occupiedOnly || v >= P.occLog) tree_write_leaf(o, P, n->leafIdx, prefix, d, col);
            continue;
        }
        int at = idx + 1, leafAt = n->leafIdx;
        for (int c = 0; c < 8; c++) {
            if (!((mask >> c) & 1u)) continue;
            const unsigned long long kid = occ_tree_kid(prefix, c);
            if (d < 15) {
                const int slot = tree_lookup(t, occ_tree_name(d + 1, kid));
                if (slot < 0) continue;                                 // only after an overflow, which the host has refused before this kernel runs
                OccTreeNode* k = t.node + slot;
                k->idx = at; k->leafIdx = leafAt;
                at += (int)(k->cnt & 0xffffffffull); leafAt += occupiedOnly ? k->nOcc : (int)(k->cnt >> 32);
            } else {
                const int slot = occ_lookup(a, kid);
                if (slot < 0) continue;
                const float kv = a.slot[slot].val; const uint32_t kc = a.slot[slot].col & OCC_WHITE;
                if (o.data && at < o.capNodes) o.data[at] = occ_tree_record(kv, kc, 0u);
                at++;
                if (!occupiedOnly || kv >= P.occLog) { tree_write_leaf(o, P, leafAt, kid, 16, kc); leafAt++; }
            }
        }
    }
}

}  // namespace

int launch_occmap_tree_up(const OccArrays& a, const OccTreeArrays& t, const OccParams& P, int prune, int innerColour, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_clear, dim3(std::max(1, std::min(divup(t.T, 256), 4096))), dim3(256), 0, s, t);
    hipLaunchKernelGGL(k_tree_voxels, dim3(std::max(1, std::min(divup(a.S, 256), 4096))), dim3(256), 0, s, a, t);
    for (int d = 15; d >= 0; d--) hipLaunchKernelGGL(k_tree_level, dim3(d >= 8 ? TREE_BLOCKS : 64), dim3(256), 0, s, a, t, d, prune, innerColour, P.occLog);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_occmap_tree_down(const OccArrays& a, const OccTreeArrays& t, const OccParams& P, int occupiedOnly, const OccTreeOut& o, hipStream_t s) {
    for (int d = 0; d <= 15; d++) hipLaunchKernelGGL(k_tree_down, dim3(d >= 8 ? TREE_BLOCKS : 64), dim3(256), 0, s, a, t, P, d, occupiedOnly, o);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
