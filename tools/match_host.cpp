// match_host.cpp — part 1 of csrc/bg_match.h (met_after, match_p, match_values, match_access,
// match_offers, match_passes, match_end_game) as a host program of its own, for
// tests/test_match_cpu.py, which builds it with AddressSanitizer and UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc tools/match_host.cpp -o match_host
// Over every score of L = 1..7, the three Crawford states, every cube byte (the invalid ones too)
// and both movers, on a grid of values (NaN and the infinities among them), three windows and
// three pairs of gammon shares, with the cubeless-play table of bgx/match.py's met_table (the same
// recurrence, here in double, rounded once) and a linear table, it checks that
//   - every lookup stays inside the tables: they are heap blocks of exactly (L + 1)^2 and L + 1
//     floats, so AddressSanitizer sees any index outside them;
//   - access implies plies > 0, craw != 1, a cube open to the mover and x > 2^k, so there is no
//     offer in a Crawford game or with a cube that is dead for the side on roll;
//   - a take gives k + 1 <= 10 owned by the taker, and the cube that was turned was below the
//     doubler's away: 2^k' / 2 < x (a cube is never turned once it is dead for the doubler);
//   - a pass, and a game played out for 1, 2 or 3 at the cube by either side, leave away in 1..L
//     and craw in 0..2, and end the match exactly when the winner's away is used up.
// It prints one line of counts and returns 1 after the first violation.
#include <math.h>
#include <stdio.h>

#include <initializer_list>
#include <vector>

#define BGX_MATCH_PART1_ONLY
#include "bg_match.h"

using namespace bg;

struct Tables {
    float* met;
    float* pc;
    int L;
    Tables(int L_) : met(new float[(L_ + 1) * (L_ + 1)]), pc(new float[L_ + 1]), L(L_) {}
    ~Tables() {
        delete[] met;
        delete[] pc;
    }
    Tables(const Tables&) = delete;
    match_tables view() const { return match_tables{met, pc, L}; }
};

// bgx/match.py met_table
static void fill_cubeless(Tables& t, double g, double b) {
    const int L = t.L, n = L + 1;
    const double r[3] = {1.0 - g - b, g, b};
    std::vector<double> pc(n, 1.0), M((size_t)n * n, 0.0);
    auto PC = [&](int j) { return j <= 0 ? 1.0 : pc[j]; };
    pc[1] = 0.5;
    for (int j = 2; j <= L; ++j) {
        double s = 0.0;
        for (int k = 1; k <= 3; ++k) s += r[k - 1] * PC(j - 2 * k);
        pc[j] = 0.5 * s;
    }
    for (int j = 0; j <= L; ++j) M[j] = 1.0;
    M[0] = 0.5;
    M[n + 1] = 0.5;
    for (int j = 2; j <= L; ++j) {
        double s = 0.0;
        for (int k = 1; k <= 3; ++k) s += r[k - 1] * (1.0 - PC(j - k));
        M[n + j] = 0.5 + 0.5 * s;
        M[(size_t)j * n + 1] = 1.0 - M[n + j];
    }
    auto Mp = [&](int a, int c) { return a <= 0 ? 1.0 : M[(size_t)a * n + c]; };
    for (int tot = 4; tot <= 2 * L; ++tot)
        for (int i = 2; i <= L; ++i) {
            const int j = tot - i;
            if (j < 2 || j > L) continue;
            double w = 0.0, l = 0.0;
            for (int k = 1; k <= 3; ++k) {
                w += r[k - 1] * Mp(i - k, j);
                l += r[k - 1] * (1.0 - Mp(j - k, i));
            }
            M[(size_t)i * n + j] = 0.5 * w + 0.5 * l;
        }
    for (int i = 0; i < n * n; ++i) t.met[i] = (float)M[i];
    for (int j = 0; j < n; ++j) t.pc[j] = (float)pc[j];
}

static void fill_linear(Tables& t) {
    const int L = t.L, n = L + 1;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) t.met[i * n + j] = 0.5f + (float)(j - i) / (float)(2 * L);
    for (int j = 0; j < n; ++j) t.pc[j] = j <= 1 ? 0.5f : 0.5f / (float)j;
    t.pc[0] = 1.0f;
}

static int fail(const char* what, int L, int x, int y, int craw, int byte, int mover) {
    fprintf(stderr, "%s: L %d x %d y %d craw %d byte %d mover %d\n", what, L, x, y, craw, byte, mover);
    return 1;
}

int main() {
    const float values[] = {-3.0f, -1.0f, -0.5f, 0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 3.0f, (float)NAN, INFINITY, -INFINITY};
    const float windows[] = {0.0f, 0.65f, 1.0f};
    const float shares[][2] = {{0.0f, 0.0f}, {0.25f, 0.25f}, {0.4f, 0.1f}};
    long cases = 0, access_n = 0, offers = 0, takes = 0, passes = 0, ends = 0, matches = 0;
    for (int L = 1; L <= 7; ++L)
        for (int table = 0; table < 2; ++table) {
            Tables tb(L);
            if (table == 0) fill_cubeless(tb, 0.26, 0.012);
            else fill_linear(tb);
            const match_tables t = tb.view();
            for (int x = 1; x <= L; ++x)
                for (int y = 1; y <= L; ++y)
                    for (int craw = 0; craw <= 2; ++craw)
                        for (int byte = 0; byte < 256; ++byte)
                            for (int mover = 0; mover < 2; ++mover) {
                                const uint8_t c = (uint8_t)byte;
                                const int k = cube_k(c, kCubeMaxCap);
                                const bool access = match_access(c, mover, 1, false, true, craw, x);
                                if (match_access(c, mover, 0, false, true, craw, x) ||
                                    match_access(c, mover, 1, true, true, craw, x) ||
                                    match_access(c, mover, 1, false, false, craw, x))
                                    return fail("access on a first ply, a finished game or an idle lane", L, x, y, craw,
                                                byte, mover);
                                if (access && (craw == 1 || x <= (1 << k) || !cube_access(c, kCubeMaxCap, mover)))
                                    return fail("access", L, x, y, craw, byte, mover);
                                access_n += access;
                                for (const float w : windows)
                                    for (const auto& sh : shares)
                                        for (const float v : values) {
                                            const match_rule r{1.0f, w, sh[0], sh[1]};
                                            // the tables are read whether or not the side has access
                                            const bool raw = match_offers(t, x, y, craw, k, r, v);
                                            const bool pass = match_passes(t, x, y, craw, k, r, v);
                                            ++cases;
                                            if (v != v && (raw || pass))
                                                return fail("a NaN offers or passes", L, x, y, craw, byte, mover);
                                            if (!(access && raw)) continue;
                                            ++offers;
                                            if (pass) {
                                                uint8_t away[2] = {(uint8_t)x, (uint8_t)y}, cr = (uint8_t)craw;
                                                const bool over = match_end_game(away, &cr, L, 0, 1ll << k);
                                                // x > 2^k: the doubler still needs points, a pass ends no match
                                                if (over || away[0] != x - (1 << k) || away[0] < 1 || away[0] > L ||
                                                    away[1] < 1 || away[1] > L || cr > 2)
                                                    return fail("pass", L, x, y, craw, byte, mover);
                                                ++passes;
                                            } else {
                                                const uint8_t next = cube_taken(c, kCubeMaxCap, mover);
                                                const int k2 = cube_k(next, kCubeMaxCap);
                                                if (k2 != k + 1 || k2 > kCubeMaxCap || cube_owner(next) != 2 - mover ||
                                                    (1 << k2) / 2 >= x)
                                                    return fail("take", L, x, y, craw, byte, mover);
                                                ++takes;
                                            }
                                        }
                                // the game played out at this cube, by either side, for 1, 2 or 3
                                for (int w = 0; w < 2; ++w)
                                    for (int s = 1; s <= 3; ++s) {
                                        uint8_t away[2] = {(uint8_t)x, (uint8_t)y}, cr = (uint8_t)craw;
                                        const long long pts = (long long)s << k;
                                        const bool over = match_end_game(away, &cr, L, w, pts);
                                        const int need = w == 0 ? x : y;
                                        if (over != (need - pts <= 0) || away[0] < 1 || away[0] > L || away[1] < 1 ||
                                            away[1] > L || cr > 2 || (over && (cr != 0 || away[0] != L || away[1] != L)) ||
                                            (!over && away[w] != need - pts))
                                            return fail("end of a game", L, x, y, craw, byte, mover);
                                        ++ends;
                                        matches += over;
                                    }
                            }
        }
    printf("cases %ld access %ld offers %ld takes %ld passes %ld ends %ld matches %ld\n", cases, access_n, offers, takes,
           passes, ends, matches);
    return 0;
}
