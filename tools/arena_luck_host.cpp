// arena_luck_host.cpp — part 1 of csrc/bg_arena_luck.h (the cubeless luck of a roll from the 21
// per-roll values, against the mid-game distribution of the rolls or the opening roll's) as a host
// program of its own, for tests/test_arena_luck_cpu.py, which builds it with AddressSanitizer and
// UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc \
//       tools/arena_luck_host.cpp -o arena_luck_host
// It reads one case per line from standard input,
//   d0 d1 opening v0 ... v20
// the 21 floats as their fp32 bit patterns in hex, and answers each with
//   luck mean
// (arena_roll_luck's two results as bit patterns).
#include <stdio.h>
#include <string.h>

#define BGX_ARENA_LUCK_PART1_ONLY
#include "bg_arena_luck.h"

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
static unsigned to_bits(float f) {
    unsigned u;
    memcpy(&u, &f, sizeof u);
    return u;
}

int main() {
    unsigned d0, d1;
    int opening;
    long cases = 0;
    while (scanf("%u %u %d", &d0, &d1, &opening) == 3) {
        float v[21], mean;
        for (int r = 0; r < 21; ++r) {
            unsigned bits;
            if (scanf("%x", &bits) != 1) {
                fprintf(stderr, "case %ld: short line\n", cases);
                return 2;
            }
            v[r] = from_bits(bits);
        }
        if (d0 > 255u || d1 > 255u) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        const float luck = bg::arena_roll_luck(v, (int)d0, (int)d1, opening, &mean);
        printf("%x %x\n", to_bits(luck), to_bits(mean));
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
