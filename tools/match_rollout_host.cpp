// match_rollout_host.cpp — part 1 of csrc/bg_match_rollout.h (match_bin, match_rollout_decision,
// the argument checks) as a host program of its own, for tests/test_match_rollout_cpu.py, which
// builds it with AddressSanitizer and UBSan:
//   g++ -O2 -g -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc tools/match_rollout_host.cpp -o match_rollout_host
// Over every score of L = 1..7, the three Crawford states, every cube byte (the invalid ones too)
// and both movers, on a grid of values (NaN and the infinities among them), three windows and
// three pairs of gammon shares, with the cubeless-play table of bgx/match.py's met_table and a
// linear table, it checks that
//   - every lookup stays inside the tables: they are heap blocks of exactly (L + 1)^2 and L + 1
//     floats, so AddressSanitizer sees any index outside them;
//   - the fused decision agrees with bg_match.h's match_access, match_offers and match_passes
//     called directly: none without access or without an offer, pass iff the answer passes, take
//     otherwise, with the next byte k + 1 owned by the taker, else the byte as it stood (sanitised);
//   - no decision but none on a first ply, a finished game, an idle lane, a NaN value, in the
//     Crawford game or with x <= 2^k;
//   - match_bin stays inside 0..87 for any kind and k, equals won * 44 + kind * 11 + k inside the
//     ranges, and maps the 88 outcomes one to one;
//   - the bin of every outcome the decision can produce (a pass at k, a game played out at k or,
//     after a take, at k + 1) is inside the histogram;
//   - the argument checks accept lengths 1..25 and valid rules only.
// It prints one line of counts and returns 1 after the first violation.
#include <math.h>
#include <stdio.h>

#include <vector>

#define BGX_MATCH_PART1_ONLY
#include "bg_match.h"
#define BGX_MATCH_ROLLOUT_PART1_ONLY
#include "bg_match_rollout.h"

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

static int check_bins() {
    bool seen[kMatchBins] = {};
    for (int won = 0; won < 2; ++won)
        for (int kind = -2; kind <= 6; ++kind)
            for (int k = -3; k <= 40; ++k) {
                const int b = match_bin(won != 0, kind, k);
                if (b < 0 || b >= kMatchBins) return fail("a bin outside 0..87", 0, kind, k, won, 0, 0);
                if (kind >= 0 && kind <= 3 && k >= 0 && k <= kCubeMaxCap) {
                    if (b != won * 44 + kind * 11 + k || seen[b]) return fail("the bin index", 0, kind, k, won, 0, 0);
                    seen[b] = true;
                }
            }
    for (bool s : seen)
        if (!s) return fail("a bin no outcome reaches", 0, 0, 0, 0, 0, 0);
    return 0;
}

static int check_args() {
    for (int L = -2; L <= 40; ++L)
        if (match_rollout_length_ok(L) != (L >= 1 && L <= 25)) return fail("length check", L, 0, 0, 0, 0, 0);
    if (match_rollout_sizes_ok(0, 1) || match_rollout_sizes_ok(1, 0) || match_rollout_sizes_ok(-1, -1) ||
        !match_rollout_sizes_ok(1, 1))
        return fail("size check", 0, 0, 0, 0, 0, 0);
    const float nan = (float)NAN;
    const match_rule good{1.0f, 0.65f, 0.25f, 0.25f};
    const match_rule bad[] = {{nan, 0.5f, 0.2f, 0.2f},  {1.0f, nan, 0.2f, 0.2f},  {1.0f, -0.1f, 0.2f, 0.2f},
                              {1.0f, 1.1f, 0.2f, 0.2f}, {1.0f, 0.5f, nan, 0.2f},  {1.0f, 0.5f, 1.5f, 0.2f},
                              {1.0f, 0.5f, 0.2f, nan},  {1.0f, 0.5f, 0.2f, -0.5f}};
    if (!match_rollout_rule_ok(good, 7) || match_rollout_rule_ok(good, 0) || match_rollout_rule_ok(good, 26))
        return fail("rule check", 0, 0, 0, 0, 0, 0);
    for (const match_rule& r : bad)
        if (match_rollout_rule_ok(r, 7)) return fail("a bad rule accepted", 0, 0, 0, 0, 0, 0);
    return 0;
}

int main() {
    if (check_bins() || check_args()) return 1;
    const float values[] = {-3.0f, -1.0f, -0.5f, 0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 3.0f, (float)NAN, INFINITY, -INFINITY};
    const float windows[] = {0.0f, 0.65f, 1.0f};
    const float shares[][2] = {{0.0f, 0.0f}, {0.25f, 0.25f}, {0.4f, 0.1f}};
    long cases = 0, nones = 0, takes = 0, passes = 0;
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
                                const uint8_t c = (uint8_t)byte, same = cube_sanitise(c, kCubeMaxCap);
                                const int k = cube_k(c, kCubeMaxCap);
                                const bool access = match_access(c, mover, 1, false, true, craw, x);
                                for (const float w : windows)
                                    for (const auto& sh : shares)
                                        for (const float v : values) {
                                            const match_rule r{1.0f, w, sh[0], sh[1]};
                                            uint8_t next = 0xFF, idle = 0xFF;
                                            const int act = match_rollout_decision(t, c, mover, 1, false, true, craw, x, y,
                                                                                   r, v, &next);
                                            ++cases;
                                            // no decision on a first ply, a finished game or an idle lane
                                            if (match_rollout_decision(t, c, mover, 0, false, true, craw, x, y, r, v, &idle) != kCubeNone ||
                                                idle != same ||
                                                match_rollout_decision(t, c, mover, 1, true, true, craw, x, y, r, v, &idle) != kCubeNone ||
                                                match_rollout_decision(t, c, mover, 1, false, false, craw, x, y, r, v, &idle) != kCubeNone)
                                                return fail("a decision without a game to decide in", L, x, y, craw, byte, mover);
                                            // bg_match.h's functions called directly
                                            const bool off = access && match_offers(t, x, y, craw, k, r, v);
                                            const bool pas = off && match_passes(t, x, y, craw, k, r, v);
                                            const int want = !off ? kCubeNone : pas ? kCubePass : kCubeTake;
                                            if (act != want) return fail("the decision", L, x, y, craw, byte, mover);
                                            if (act != kCubeNone && (v != v || craw == 1 || x <= (1 << k)))
                                                return fail("a double on a NaN, in the Crawford game or with a dead cube", L,
                                                            x, y, craw, byte, mover);
                                            if (act == kCubeTake) {
                                                if (next != cube_taken(c, kCubeMaxCap, mover) || cube_k(next, kCubeMaxCap) != k + 1 ||
                                                    k + 1 > kCubeMaxCap || cube_owner(next) != 2 - mover)
                                                    return fail("take", L, x, y, craw, byte, mover);
                                                ++takes;
                                            } else if (next != same) {
                                                return fail("the byte after none or a pass", L, x, y, craw, byte, mover);
                                            }
                                            passes += act == kCubePass;
                                            nones += act == kCubeNone;
                                            // the bins this step's outcomes go to
                                            const int kend = cube_k(next, kCubeMaxCap);
                                            for (int won = 0; won < 2; ++won)
                                                for (int kind = 0; kind <= 3; ++kind) {
                                                    const int b = match_bin(won != 0, kind, kind == 0 ? k : kend);
                                                    if (b < 0 || b >= kMatchBins || b / 44 != won || b % 44 / 11 != kind)
                                                        return fail("an outcome's bin", L, x, y, craw, byte, mover);
                                                }
                                        }
                            }
        }
    printf("cases %ld nones %ld takes %ld passes %ld\n", cases, nones, takes, passes);
    return takes > 0 && passes > 0 ? 0 : 1;
}
