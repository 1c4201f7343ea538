// cube_host.cpp — part 1 of csrc/bg_cube.h (the cube's state byte and the decision rule) as a
// host program of its own, for tests/test_cube_cpu.py, which builds it with AddressSanitizer and
// UBSan:
//   g++ -O2 -g -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc tools/cube_host.cpp -o cube_host
// It reads one case per line from standard input,
//   byte cap mover scale equity double_at pass_at too_good_at
// the five floats as their fp32 bit patterns in hex, and answers each with
//   action next access k owner
// (cube_decision's result and *next, cube_access, cube_k, cube_owner).
#include <stdio.h>
#include <string.h>

#define BGX_CUBE_PART1_ONLY
#include "bg_cube.h"

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

int main() {
    unsigned byte, bits[5];
    int cap, mover;
    long cases = 0;
    while (scanf("%u %d %d %x %x %x %x %x", &byte, &cap, &mover, &bits[0], &bits[1], &bits[2], &bits[3], &bits[4]) == 8) {
        if (byte > 255u || cap < 0 || cap > bg::kCubeMaxCap || (mover != 0 && mover != 1)) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        uint8_t next = 0;
        const int action = bg::cube_decision((uint8_t)byte, cap, mover, from_bits(bits[0]), from_bits(bits[1]),
                                             from_bits(bits[2]), from_bits(bits[3]), from_bits(bits[4]), &next);
        printf("%d %d %d %d %d\n", action, (int)next, (int)bg::cube_access((uint8_t)byte, cap, mover),
               bg::cube_k((uint8_t)byte, cap), bg::cube_owner((uint8_t)byte));
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
