// cube_trunc_host.cpp — part 1 of csrc/bg_cube_trunc.h (Janowski's rule: the four values and the
// flags from a cube byte, a mover and a cubeless value; the cut's fixed point) as a host program
// of its own, for tests/test_cube_truncate_cpu.py, which builds it with AddressSanitizer and
// UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc \
//       tools/cube_trunc_host.cpp -o cube_trunc_host
// It reads one case per line from standard input,
//   byte cap mover start_mover jacoby scale v x W L
// the five floats as their fp32 bit patterns in hex, and answers each with
//   k flags nd dt e c yq
// (cube_k, cube_trunc_values' flags and four values as bit patterns, and cube_trunc_q of e).
#include <stdio.h>
#include <string.h>

#define BGX_CUBE_TRUNC_PART1_ONLY
#include "bg_cube_trunc.h"

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
    unsigned byte, bits[5];
    int cap, mover, start, jacoby;
    long cases = 0;
    while (scanf("%u %d %d %d %d %x %x %x %x %x", &byte, &cap, &mover, &start, &jacoby, &bits[0], &bits[1], &bits[2],
                 &bits[3], &bits[4]) == 10) {
        const float x = from_bits(bits[2]), W = from_bits(bits[3]), L = from_bits(bits[4]);
        if (byte > 255u || cap < 0 || cap > bg::kCubeMaxCap || (mover != 0 && mover != 1) || (start != 0 && start != 1) ||
            !bg::cube_life_ok(x, W, L)) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        const int k = bg::cube_k((uint8_t)byte, cap);
        float v[4];
        const int flags = bg::cube_trunc_values((uint8_t)byte, cap, mover, from_bits(bits[0]), from_bits(bits[1]), x, W, L,
                                                jacoby, v);
        const long long yq = bg::cube_trunc_q(v[2], mover == start, k);
        printf("%d %d %x %x %x %x %lld\n", k, flags, to_bits(v[0]), to_bits(v[1]), to_bits(v[2]), to_bits(v[3]), yq);
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
