// N-split tiles of the fused 4-chain stream (flow_r4f.h; density sections of the fp32 image): which (k-quad, column) the float4 of
// lane `lane` in tile g of wave w of item I holds.  Plain C++ on purpose - k_pack_r4f lays the image out with it and
// tests/test_r4f_nsplit_map.py compiles it into a host program.
#pragma once
#ifndef FAB_HD
#define FAB_HD inline
#endif

namespace fab {

// Items 0, 1 (S1: fused W1', S4: W3^T; K = 32 = 8 k-quads) and 3 .. 4 G + 2 (S2: W2, S5: W2^T; K = 64 G = 16 G k-quads), G = hidden
// width / 64.  Lane quarter Q = lane >> 4 of EVERY wave multiplies the k-quads wave Q multiplies in the K-split layout, in the same
// order (item by item); wave w does so for the 16 G columns it owns, tile g = columns 16 G w + 16 g .. + 15.
FAB_HD void r4f_nsplit_kn(int G, int I, int w, int g, int lane, int& q, int& n) {
    const int Q = lane >> 4, c = lane & 15;
    q = I < 2 ? 2 * Q + I : 4 * G * Q + (I - 3);
    n = 16 * G * w + 16 * g + c;
}

}  // namespace fab
