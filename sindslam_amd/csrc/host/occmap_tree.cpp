// Host twin of sind_occmap_tree / sind_occmap_write_ot (include/sind_hip.h): the LITERAL form.  A pointer tree built from the twin's flat map, octomap's prune() loop
// (pruneRecurs per depth from 15 down to 1, the `depth > 0` that spares the root and the early break on a depth that pruned nothing), the recursive
// updateInnerOccupancy (updateOccupancyChildren always: octomap keeps inner values current while it inserts; updateColorChildren only when asked, because the reference
// never calls it), the recursive writeNodesRecurs and a recursive walk over the leaves.  It shares the arithmetic of occmap_tree.hpp with the device and nothing of its
// schedule (no levels, no table of nodes, no integer images: values are compared as floats).
//   Order: prune, then updateInnerOccupancy.  The other order gives the same tree: the average colour of eight equal children is that colour (or white for white), and
// the maximum of eight equal values is that value, which is what pruneNode copies from child 0.
#include <cstring>
#include <deque>
#include <vector>
#include "occmap_tree.hpp"
#include "occmap_twin.hpp"
#include "sind_hip.h"

using namespace sind;

static_assert(sizeof(sind_occmap_tree_stats) == sizeof(OccTreeStats), "the ABI struct is the shared struct");

namespace {

struct Node { float v = 0.0f; uint32_t col = OCC_WHITE; Node* ch[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; };

struct Tree {
    std::deque<Node> pool; Node* root = nullptr; int nPruned = 0;
    Node* make() { pool.emplace_back(); return &pool.back(); }
    static bool hasChildren(const Node* n) { for (int i = 0; i < 8; i++) if (n->ch[i]) return true; return false; }

    void set(int kx, int ky, int kz, float v, uint32_t col) {
        if (!root) root = make();
        Node* n = root;
        for (int d = 0; d < OCC_TREE_DEPTH; d++) { Node*& c = n->ch[occ_tree_child(kx, ky, kz, d)]; if (!c) c = make(); n = c; }
        n->v = v; n->col = col;
    }
    // isNodeCollapsible / pruneNode
    static bool collapsible(const Node* n) {
        const Node* first = n->ch[0];
        if (!first || hasChildren(first)) return false;
        for (int i = 1; i < 8; i++) {
            const Node* c = n->ch[i];
            if (!c || hasChildren(c) || !(c->v == first->v && c->col == first->col)) return false;
        }
        return true;
    }
    bool pruneNode(Node* n) {
        if (!collapsible(n)) return false;
        n->v = n->ch[0]->v; n->col = n->ch[0]->col;
        for (int i = 0; i < 8; i++) n->ch[i] = nullptr;
        return true;
    }
    void pruneRecurs(Node* n, int depth, int maxDepth, int& num) {
        if (depth < maxDepth) { for (int i = 0; i < 8; i++) if (n->ch[i]) pruneRecurs(n->ch[i], depth + 1, maxDepth, num); }
        else if (pruneNode(n)) num++;
    }
    void prune() {
        if (!root) return;
        for (int depth = OCC_TREE_DEPTH - 1; depth > 0; --depth) {
            int num = 0;
            pruneRecurs(root, 0, depth, num);
            if (num == 0) break;
            nPruned += num;
        }
    }
    void updateInner(Node* n, int depth, bool colour) {
        if (!hasChildren(n)) return;
        if (depth < OCC_TREE_DEPTH) for (int i = 0; i < 8; i++) if (n->ch[i]) updateInner(n->ch[i], depth + 1, colour);
        bool any = false; float m = 0.0f; uint64_t sums = 0;
        for (int i = 0; i < 8; i++) {
            const Node* c = n->ch[i];
            if (!c) continue;
            if (!any || c->v > m) m = c->v;
            any = true; sums += occ_tree_colour_term(c->col);
        }
        n->v = m; n->col = colour ? occ_tree_colour_average(sums) : OCC_WHITE;
    }
};

struct Walk {
    const OccParams* P; float occLog; bool occupiedOnly;
    OccTreeStats st{}; int nListed = 0;
    uint8_t* data = nullptr; sind_cloud_point* leaves = nullptr; uint8_t* leafDepth = nullptr;
    // writeNodesRecurs and the leaf walk in one recursion; with no outputs it only counts
    void node(const Node* n, int depth, int kx, int ky, int kz) {
        uint32_t mask = 0;
        for (int i = 0; i < 8; i++) if (n->ch[i]) mask |= 1u << i;
        if (data) { const uint64_t rec = occ_tree_record(n->v, n->col, mask); std::memcpy(data + 8 * (size_t)st.nNodes, &rec, 8); }
        st.nNodes++;
        if (!mask) {
            st.nLeaves++; st.leavesAtDepth[depth]++;
            const bool occ = n->v >= occLog; st.nOccupiedLeaves += occ;
            if (occ || !occupiedOnly) {
                if (leaves) {
                    sind_cloud_point& p = leaves[nListed];
                    p.x = occ_tree_centre(*P, kx, depth); p.y = occ_tree_centre(*P, ky, depth); p.z = occ_tree_centre(*P, kz, depth);
                    p.r = n->col & 255; p.g = (n->col >> 8) & 255; p.b = (n->col >> 16) & 255; p.a = 0;
                }
                if (leafDepth) leafDepth[nListed] = (uint8_t)depth;
                nListed++;
            }
            return;
        }
        st.nInner++;
        const int s = 15 - depth;
        for (int i = 0; i < 8; i++) if (n->ch[i]) node(n->ch[i], depth + 1, kx | ((i & 1) << s), ky | (((i >> 1) & 1) << s), kz | (((i >> 2) & 1) << s));
    }
};

void build(sindh_occmap* h, int prune, int innerColour, Tree& t) {
    for (const auto& kv : h->map) {
        if (!kv.second.known) continue;
        const OccVoxel& x = kv.second;
        t.set((int)(kv.first & 0xffff), (int)((kv.first >> 16) & 0xffff), (int)((kv.first >> 32) & 0xffff), x.v, (uint32_t)x.r | ((uint32_t)x.g << 8) | ((uint32_t)x.b << 16));
    }
    if (prune) t.prune();
    if (t.root) t.updateInner(t.root, 0, innerColour != 0);
}

}  // namespace

extern "C" {

int sindh_occmap_tree(sindh_occmap* h, int prune, int inner_colour, int occupied_only, uint8_t* data, size_t cap_bytes, sind_cloud_point* leaves, uint8_t* leaf_depth,
                      int cap_leaves, int* n_leaves_out, sind_occmap_tree_stats* stats) {
    if (!h || !stats || (leaves && cap_leaves < 0) || (leaf_depth && !leaves)) return SIND_E_ARG;
    Tree t; build(h, prune, inner_colour, t);
    Walk count; count.P = &h->P; count.occLog = h->P.occLog; count.occupiedOnly = occupied_only != 0;
    if (t.root) count.node(t.root, 0, 0, 0, 0);
    count.st.nPruned = t.nPruned;
    std::memcpy(stats, &count.st, sizeof(OccTreeStats));
    if (n_leaves_out) *n_leaves_out = count.nListed;
    if ((data && (size_t)count.st.nNodes * 8 > cap_bytes) || (leaves && count.nListed > cap_leaves)) return SIND_E_CAPACITY;
    if ((!data && !leaves) || !t.root) return SIND_OK;
    Walk w; w.P = &h->P; w.occLog = h->P.occLog; w.occupiedOnly = count.occupiedOnly; w.data = data; w.leaves = leaves; w.leafDepth = leaf_depth;
    w.node(t.root, 0, 0, 0, 0);
    return SIND_OK;
}

int sindh_occmap_write_ot(sindh_occmap* h, int prune, int inner_colour, const char* path) {
    if (!h || !path) return SIND_E_ARG;
    sind_occmap_tree_stats st;
    int rc = sindh_occmap_tree(h, prune, inner_colour, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, &st);
    if (rc != SIND_OK) return rc;
    std::vector<uint8_t> data((size_t)st.n_nodes * 8);
    if (st.n_nodes) { rc = sindh_occmap_tree(h, prune, inner_colour, 0, data.data(), data.size(), nullptr, nullptr, 0, nullptr, &st); if (rc != SIND_OK) return rc; }
    return occ_tree_write_file(path, occ_tree_ot_header(st.n_nodes, h->P.res), data.data(), data.size()) ? SIND_OK : SIND_E_ARG;
}

}  // extern "C"
