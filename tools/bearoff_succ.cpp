// bearoff_succ.cpp — the bearoff database's successor enumeration (part 1 of
// csrc/bg_bearoff.h, plain C++) as a host program: for every configuration of at most K
// checkers and each of the 21 rolls, one line
//     key r0 r1 count key_1 ... key_count
// with the base-9 keys (sum_d c[d-1] 9^(d-1)) of the configuration and of its successors,
// ascending.  tests/test_bearoff_cpu.py builds it with AddressSanitizer + UBSan and compares
// the sets with the oracle's move generator.
//     c++ -O1 -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc tools/bearoff_succ.cpp -o bearoff_succ
#define BGX_BEAROFF_HOST_ONLY
#include "bg_bearoff.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

using namespace bg;

int main(int argc, char** argv) {
    const int K = argc > 1 ? atoi(argv[1]) : 4;
    if (K < 1 || K > kBoMaxK) return 2;
    int c[6], widest = 0;
    long total = 0;
    for (c[0] = 0; c[0] <= K; ++c[0]) for (c[1] = 0; c[0] + c[1] <= K; ++c[1])
    for (c[2] = 0; c[0] + c[1] + c[2] <= K; ++c[2]) for (c[3] = 0; c[0] + c[1] + c[2] + c[3] <= K; ++c[3])
    for (c[4] = 0; c[0] + c[1] + c[2] + c[3] + c[4] <= K; ++c[4])
    for (c[5] = 0; c[0] + c[1] + c[2] + c[3] + c[4] + c[5] <= K; ++c[5]) {
        uint32_t pack = 0;
        for (int d = 1; d <= 6; ++d) pack |= (uint32_t)c[d - 1] << (4 * (d - 1));
        for (int r = 0; r < kBoRolls; ++r) {
            int r0, r1;
            bo_roll(r, r0, r1);
            BoSet s;
            const int m = bo_successors(pack, r0, r1, s);
            if (s.ovf) { fprintf(stderr, "successor set overflow\n"); return 1; }
            int keys[kBoSetCap];
            for (int i = 0; i < m; ++i) keys[i] = bo_key(s.pack[i]);
            std::sort(keys, keys + m);
            printf("%d %d %d %d", bo_key(pack), r0, r1, m);
            for (int i = 0; i < m; ++i) printf(" %d", keys[i]);
            printf("\n");
            widest = std::max(widest, m);
            total += m;
        }
    }
    fprintf(stderr, "K %d widest %d total %ld\n", K, widest, total);
    return 0;
}
