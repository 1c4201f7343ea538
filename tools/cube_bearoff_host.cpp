// cube_bearoff_host.cpp — part 1 of csrc/bg_bearoff_cube.h (the cube state of a record's mover,
// the choice of the lookup's values and flags, the cut's fixed point) as a host program of its
// own, for tests/test_cube_bearoff_cpu.py, which builds it with AddressSanitizer and UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc \
//       tools/cube_bearoff_host.cpp -o cube_bearoff_host
// It reads one case per line from standard input,
//   byte cap mover start_mover plies nd_cen nd_own e_opp w
// the four floats as their fp32 bit patterns in hex, and answers each with
//   state k flags nd dt e cubeless yq
// (boc_state, cube_k, boc_values' flags and four values as bit patterns, and boc_fixed of nd on
// the first ply, plies == 0, else of e).
#include <stdio.h>
#include <string.h>

#define BGX_CUBE_PART1_ONLY
#include "bg_bearoff_cube.h"

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
    unsigned byte, bits[4];
    int cap, mover, start, plies;
    long cases = 0;
    while (scanf("%u %d %d %d %d %x %x %x %x", &byte, &cap, &mover, &start, &plies, &bits[0], &bits[1], &bits[2],
                 &bits[3]) == 9) {
        if (byte > 255u || cap < 0 || cap > bg::kCubeMaxCap || (mover != 0 && mover != 1) || (start != 0 && start != 1) ||
            plies < 0) {
            fprintf(stderr, "case %ld: out of range\n", cases);
            return 2;
        }
        const int state = bg::boc_state((uint8_t)byte, cap, mover), k = bg::cube_k((uint8_t)byte, cap);
        const float nd_s = state == bg::kBocCen ? from_bits(bits[0]) : state == bg::kBocOwn ? from_bits(bits[1]) : 0.0f;
        float v[4];
        const int flags = bg::boc_values(state, nd_s, from_bits(bits[2]), from_bits(bits[3]), v);
        const long long yq = bg::boc_fixed(plies == 0 ? v[0] : v[2], mover == start, k);
        printf("%d %d %d %x %x %x %x %lld\n", state, k, flags, to_bits(v[0]), to_bits(v[1]), to_bits(v[2]), to_bits(v[3]),
               yq);
        ++cases;
    }
    fprintf(stderr, "cases %ld\n", cases);
    return 0;
}
