// Host check of bgx_roll_luck's workspace layout (csrc/bg_workspace.h LuckLayout): built with
// -fsanitize=address,undefined and run by tests/test_rollout_luck_cpu.py.
#include <stdio.h>
#include <initializer_list>

#include "bg_workspace.h"

using namespace bgws;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// floats of a value pack of NT 16-unit slices (csrc/bg_search.hip sz_f16)
static size_t pack_floats(int NT) { return 4 + 13 * (size_t)slices(NT) * 64 * 4 + (size_t)slices(NT) * 8 * 64; }

int main() {
    const size_t kMostRows = (0x1FFFFFFF - 1) / 21;
    for (size_t B : {1, 3, 64, 256, 65536})
        for (size_t rows : {(size_t)1, (size_t)63, (size_t)256, (size_t)65536, kMostRows})
            for (int NT = 1; NT <= 8; ++NT) {
                TwoPlyLayout L(B);
                L.body(rows, rows * 21, NT, false);
                const LuckLayout K(L.bytes(), pack_floats(NT));
                // behind the 2-ply regions, on a 256-byte boundary, and nothing of the 2-ply layout moves
                EXPECT(K.start() == L.bytes() && K.pack.off == K.start() && K.pack.off % 256 == 0, "B %zu rows %zu", B, rows);
                EXPECT(K.pack.off >= L.rowpart.off + L.rowpart.bytes(), "the pack overlaps rowpart");
                EXPECT(K.pack.count == pack_floats(NT), "NT %d", NT);
                EXPECT(K.bytes() == align_up(K.pack.off + K.pack.bytes()) && K.bytes() % 256 == 0, "bytes() %zu", K.bytes());
                // the evaluators read w1q as 16-byte words at pack + 4 floats
                EXPECT((K.pack.off + 16) % 16 == 0, "w1q alignment");
            }
    // an unaligned start is rounded up
    const LuckLayout U(1000, 10);
    EXPECT(U.start() == 1024 && U.pack.off == 1024 && U.bytes() == 1280, "%zu %zu", U.start(), U.bytes());
    // H = 128: 13 k-blocks x 8 slices x 64 lanes x 16 B of weights + 8 x 8 x 64 head weights + the header
    EXPECT(pack_floats(8) == 30724 && LuckLayout(0, pack_floats(8)).bytes() == 123136, "%zu", LuckLayout(0, pack_floats(8)).bytes());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("luck workspace ok\n");
    return 0;
}
