// cube_luck_host.cpp — part 1 of csrc/bg_cube_luck.h (the cubeful luck of a roll from the 21
// per-roll values: Janowski's equity after each roll with the opponent on roll, the FMA chain of
// the mean, the luck; a game's luck in fixed point) as a host program of its own, for
// tests/test_cube_luck_cpu.py, which builds it with AddressSanitizer and UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc \
//       tools/cube_luck_host.cpp -o cube_luck_host
// It reads one case per line from standard input,
//   byte cap mover jacoby d0 d1 scale x W L sum v0 ... v20
// the 26 floats as their fp32 bit patterns in hex, and answers each with
//   luck mean lq
// (cube_roll_luck's two results as bit patterns, and cube_luck_q of `sum`).
#include <stdio.h>
#include <string.h>

#define BGX_CUBE_LUCK_PART1_ONLY
#include "bg_cube_luck.h"

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
    unsigned byte, d0, d1;
    int cap, mover, jacoby;
    long cases = 0;
    while (scanf("%u %d %d %d %u %u", &byte, &cap, &mover, &jacoby, &d0, &d1) == 6) {
        unsigned bits[26];
        for (int k = 0; k < 26; ++k)
            if (scanf("%x", &bits[k]) != 1) {
                fprintf(stderr, "case %ld: short line\n", cases);
                return 2;
            }
        const float scale = from_bits(bits[0]), x = from_bits(bits[1]), W = from_bits(bits[2]), L = from_bits(bits[3]);
        if (byte > 255u || cap < 0 || cap > bg::kCubeMaxCap || (mover != 0 && mover != 1) || d0 > 255u || d1 > 255u ||
            scale != scale || !bg::cube_life_ok(x, W, L)) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        float v[21], mean;
        for (int r = 0; r < 21; ++r) v[r] = from_bits(bits[5 + r]);
        const float luck = bg::cube_roll_luck(v, (uint8_t)byte, cap, mover, (int)d0, (int)d1, scale, x, W, L, jacoby, &mean);
        printf("%x %x %lld\n", to_bits(luck), to_bits(mean), bg::cube_luck_q(from_bits(bits[4])));
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
