// The host twin's map (sindh_occmap_*): a flat hash map of known voxels.  Shared by csrc/host/occmap.cpp (insert and the flat queries) and csrc/host/occmap_tree.cpp
// (the snapshot tree), which are separate translation units.
#pragma once
#include <unordered_map>
#include "occmap.hpp"

struct sindh_occmap { sind::OccParams P; int maxVoxels, maxPoints; std::unordered_map<uint64_t, sind::OccVoxel> map; };
