// Launchers of csrc/covis_kernels.hip (the covisibility table, include/sind_hip.h "sind_covis_*"); every pointer is a device pointer.
#pragma once
#include "common.hpp"
#include "host/covis.hpp"

namespace sind {

int launch_covis_apply(const CovisTable& t, const ::sind_covis_op* ops, int n, hipStream_t s);
// tag / untag the n entries (point, bit) in tag [words][capPoints]
int launch_covis_tag(unsigned long long* tag, const int* entPoint, const int* entBit, int n, int capPoints, bool set, hipStream_t s);
// perBit[bit * rows + kf] = the cells of row kf whose point carries the bit, for kf < rows and bit < nBits
int launch_covis_count(const CovisTable& t, const unsigned long long* tag, int* perBit, int rows, int nBits, hipStream_t s);
// n entries of B items, item b = entries itemStart[b] .. itemStart[b + 1] - 1 of key frame itemKf[b]; counts [B][2] = (n_mps, n_redundant) must be 0 on entry
int launch_covis_cull(const CovisTable& t, const int* itemStart, const int* itemKf, int B, const int* entPoint, const uint8_t* entOctave, const uint8_t* entClose, int n,
                      int thObs, int* counts, uint8_t* redundant, hipStream_t s);

}  // namespace sind
