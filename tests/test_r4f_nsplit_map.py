"""The (item, wave, tile, lane) -> (k-quad, column) map of the N-split tiles of the fused 4-chain stream (csrc/r4f_nsplit_map.h:
what k_pack_r4f lays the density sections of the fp32 image out with), compiled into a host program - no GPU.  For G = 2, 4, 5:
the tiles of S1 / S4 (items 0, 1; 8 k-quads) and of S2 / S5 (items 3 .. 4 G + 2; 16 G k-quads) cover every (k-quad, column) of the
matrix exactly once, wave w holds columns [16 G w, 16 G (w + 1)) only, and lane quarter Q gets exactly the k-quads wave Q has in
the K-split layout (2 Q, 2 Q + 1 / 4 G Q .. 4 G Q + 4 G - 1), in ascending item order."""
import os
import subprocess

from fab_torch_amd import _build

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "r4f_nsplit_map.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// items [I0, I0 + NI) of a stage with NQ k-quads: coverage, column ownership, k order per lane quarter
static void stage(int G, int I0, int NI, int NQ, int per_quarter) {
    const int N = 64 * G;
    std::vector<int> seen((size_t)NQ * N, 0);
    for (int w = 0; w < 4; ++w)
        for (int g = 0; g < G; ++g)
            for (int lane = 0; lane < 64; ++lane) {
                const int Q = lane >> 4;
                for (int i = 0; i < NI; ++i) {
                    int q = -1, n = -1;
                    fab::r4f_nsplit_kn(G, I0 + i, w, g, lane, q, n);
                    CHECK(q >= 0 && q < NQ && n >= 0 && n < N, "G %d item %d w %d g %d lane %d: (%d, %d) out of range", G, I0 + i, w, g, lane, q, n);
                    if (q < 0 || q >= NQ || n < 0 || n >= N) continue;
                    ++seen[(size_t)q * N + n];
                    CHECK(n == 16 * G * w + 16 * g + (lane & 15), "G %d item %d w %d g %d lane %d: column %d", G, I0 + i, w, g, lane, n);
                    CHECK(n >= 16 * G * w && n < 16 * G * (w + 1), "G %d w %d: column %d is not the wave's own", G, w, n);
                    // former wave Q's k-quads, ascending with the item
                    CHECK(q == per_quarter * Q + i, "G %d item %d lane %d: k-quad %d, wave %d's is %d", G, I0 + i, lane, q, Q, per_quarter * Q + i);
                }
            }
    for (int q = 0; q < NQ; ++q)
        for (int n = 0; n < N; ++n)
            CHECK(seen[(size_t)q * N + n] == 1, "G %d items %d..: (k-quad %d, column %d) covered %d times", G, I0, q, n, seen[(size_t)q * N + n]);
}

int main() {
    const int Gs[3] = {2, 4, 5};
    for (int G : Gs) {
        stage(G, 0, 2, 8, 2);                  // S1 / S4: K = 32
        stage(G, 3, 4 * G, 16 * G, 4 * G);     // S2 / S5: K = 64 G
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def test_nsplit_tiles_cover_the_matrices_once_and_keep_each_waves_k_order(tmp_path):
    src, exe = tmp_path / "nsplit_map_check.cpp", tmp_path / "nsplit_map_check"
    src.write_text(PROGRAM)
    r = subprocess.run([_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-I", _build.CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, f"compiling the map check failed:\n{r.stderr[-4000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")
