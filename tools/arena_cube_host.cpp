// arena_cube_host.cpp — part 1 of csrc/bg_arena_cube.h (cube_offers, cube_passes, cube_taken) as
// a host program of its own, for tests/test_arena_cube_cpu.py, which builds it with
// AddressSanitizer and UBSan:
//   g++ -O2 -g -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc tools/arena_cube_host.cpp -o arena_cube_host
// The identity it checks: with one rule and one equity for both halves, offer followed by respond
// is cube_decision -- its action and its next byte -- for every state byte (the invalid ones
// too), both movers, the caps 0..10, three threshold sets and equities on, beside and far from
// the thresholds, NaN and the infinities.  It prints the number of cases and of each action and
// returns 1 after the first mismatch.
#include <math.h>
#include <stdio.h>

#include <initializer_list>

#define BGX_CUBE_PART1_ONLY
#include "bg_arena_cube.h"

struct Rule { float scale, double_at, pass_at, too_good_at; };

int main() {
    const Rule rules[] = {{1.0f, 0.4f, 0.5f, INFINITY}, {1.5f, 0.3f, 0.6f, 0.9f}, {1.0f, INFINITY, INFINITY, INFINITY},
                          {-1.0f, -0.2f, 0.1f, 0.3f}};
    long cases = 0, actions[3] = {0, 0, 0};
    for (const Rule& r : rules) {
        float eqs[64];
        int ne = 0;
        for (float th : {r.double_at, r.pass_at, r.too_good_at}) {
            const float x = th / r.scale;               // the equity whose product is the threshold, and its neighbours
            for (float v : {x, nextafterf(x, -INFINITY), nextafterf(x, INFINITY), th}) eqs[ne++] = v;
        }
        for (float v : {-3.0f, -1.0f, -0.0f, 0.0f, 0.45f, 0.95f, 3.0f, (float)NAN, INFINITY, -INFINITY}) eqs[ne++] = v;
        for (int cap = 0; cap <= bg::kCubeMaxCap; ++cap)
            for (int byte = 0; byte < 256; ++byte)
                for (int mover = 0; mover < 2; ++mover)
                    for (int j = 0; j < ne; ++j) {
                        const uint8_t c = (uint8_t)byte;
                        uint8_t want_next = 0;
                        const int want = bg::cube_decision(c, cap, mover, r.scale, eqs[j], r.double_at, r.pass_at,
                                                           r.too_good_at, &want_next);
                        int got = bg::kCubeNone;
                        uint8_t next = bg::cube_sanitise(c, cap);
                        if (bg::cube_offers(c, cap, mover, r.scale, eqs[j], r.double_at, r.too_good_at)) {
                            got = bg::cube_passes(r.scale, eqs[j], r.pass_at) ? bg::kCubePass : bg::kCubeTake;
                            if (got == bg::kCubeTake) next = bg::cube_taken(c, cap, mover);
                        }
                        if (got != want || next != want_next) {
                            fprintf(stderr, "mismatch: byte %d cap %d mover %d equity %a: %d %d, cube_decision %d %d\n",
                                    byte, cap, mover, (double)eqs[j], got, (int)next, want, (int)want_next);
                            return 1;
                        }
                        if (got == bg::kCubeTake && (bg::cube_k(next, cap) != bg::cube_k(c, cap) + 1 ||
                                                     bg::cube_owner(next) != 2 - mover || bg::cube_k(next, cap) > cap)) {
                            fprintf(stderr, "take: byte %d cap %d mover %d -> %d\n", byte, cap, mover, (int)next);
                            return 1;
                        }
                        ++actions[got];
                        ++cases;
                    }
    }
    printf("cases %ld none %ld take %ld pass %ld\n", cases, actions[0], actions[1], actions[2]);
    return 0;
}
