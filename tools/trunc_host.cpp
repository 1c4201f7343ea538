// trunc_host.cpp — part 1 of csrc/bg_trunc.h (a truncated game's fixed-point result) as a host
// program of its own, for tests/test_truncate_cpu.py, which builds it with AddressSanitizer and
// UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc
//       tools/trunc_host.cpp -o trunc_host
// It reads one case per line from standard input,
//   scale value same
// the two floats as their fp32 bit patterns in hex, `same` 0 or 1, and answers each with Vq
// (trunc_value_q's result).
#include <stdio.h>
#include <string.h>

#define BGX_TRUNC_PART1_ONLY
#include "bg_trunc.h"

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

int main() {
    unsigned bits[2];
    int same;
    long cases = 0;
    while (scanf("%x %x %d", &bits[0], &bits[1], &same) == 3) {
        if (same != 0 && same != 1) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        printf("%lld\n", bg::trunc_value_q(from_bits(bits[0]), from_bits(bits[1]), same != 0));
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
