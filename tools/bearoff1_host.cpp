// bearoff1_host.cpp — the one-sided bearoff database's host-and-device code (csrc/bg_bearoff1.h
// on part 1 of csrc/bg_bearoff.h, plain C++) as a host program.  tests/test_bearoff1_cpu.py
// builds it with AddressSanitizer + UBSan.
//     c++ -O2 -ffp-contract=off -fsanitize=address,undefined -I mlp-ppo-2ply-p3_amd/csrc \
//         tools/bearoff1_host.cpp -o bearoff1_host
//   bearoff1_host succ K    (K <= 8) for every configuration and roll, the distinct plays of
//       bo_visit with the largest number of sub-moves against bo_successors' set; prints
//       "K sets mismatches widest"
//   bearoff1_host table K   (K <= 15) the whole table by the recurrence of include/bgx.h in
//       fp32, with B1Argmin as the device uses it; prints n, the largest and the total size of
//       the successor sets, the (configuration, roll) pairs with a tie at the minimum, the last
//       t with a non-zero entry, the smallest and largest row sum (fp64 sums of the fp32
//       entries) and the means of six and of K checkers on the six point, with their bits
#define BGX_BEAROFF_HOST_ONLY
#include "bg_bearoff1.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

using namespace bg;

struct Config { int pip; uint32_t pack; };

static std::vector<Config> configs_of(int K) {
    std::vector<Config> cfg;
    int c[6];
    for (c[0] = 0; c[0] <= K; ++c[0]) for (c[1] = 0; c[0] + c[1] <= K; ++c[1])
    for (c[2] = 0; c[0] + c[1] + c[2] <= K; ++c[2]) for (c[3] = 0; c[0] + c[1] + c[2] + c[3] <= K; ++c[3])
    for (c[4] = 0; c[0] + c[1] + c[2] + c[3] + c[4] <= K; ++c[4])
    for (c[5] = 0; c[0] + c[1] + c[2] + c[3] + c[4] + c[5] <= K; ++c[5]) {
        Config x{0, 0u};
        for (int d = 1; d <= 6; ++d) { x.pip += d * c[d - 1]; x.pack |= (uint32_t)c[d - 1] << (4 * (d - 1)); }
        cfg.push_back(x);
    }
    std::sort(cfg.begin(), cfg.end(), [](const Config& a, const Config& b) {
        return a.pip != b.pip ? a.pip < b.pip : a.pack < b.pack;
    });
    return cfg;
}

// the plays of the largest length, as a sorted set
struct Collect {
    std::vector<uint32_t> packs;
    int len = 0;
    void operator()(uint32_t pack, int l) {
        if (l < len) return;
        if (l > len) { packs.clear(); len = l; }
        packs.push_back(pack);
    }
    void finish() {
        std::sort(packs.begin(), packs.end());
        packs.erase(std::unique(packs.begin(), packs.end()), packs.end());
    }
};

static int run_succ(int K) {
    if (K > kBoMaxK) return 2;
    long sets = 0, mismatches = 0;
    size_t widest = 0;
    for (const Config& x : configs_of(K)) {
        for (int r = 0; r < kBoRolls; ++r) {
            int r0, r1;
            bo_roll(r, r0, r1);
            BoSet s;
            const int m = bo_successors(x.pack, r0, r1, s);
            if (s.ovf) { fprintf(stderr, "successor set overflow\n"); return 1; }
            std::vector<uint32_t> want(s.pack, s.pack + m);
            std::sort(want.begin(), want.end());
            Collect got;
            bo_visit(x.pack, r0, r1, got);
            got.finish();
            if (got.packs.empty()) got.packs.push_back(x.pack);       // a roll that cannot be played
            mismatches += got.packs != want;
            widest = std::max(widest, got.packs.size());
            ++sets;
        }
    }
    printf("K %d sets %ld mismatches %ld widest %zu\n", K, sets, mismatches, widest);
    return mismatches ? 1 : 0;
}

static int run_table(int K) {
    const std::vector<Config> cfg = configs_of(K);
    const int n = (int)cfg.size();
    std::vector<int32_t> index_of((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        const int rk = b1_rank(cfg[i].pack, K);
        if (rk < 0 || rk >= n || index_of[rk] >= 0) { fprintf(stderr, "rank of %x: %d\n", cfg[i].pack, rk); return 1; }
        index_of[rk] = i;
    }
    std::vector<float> dist((size_t)n * kB1T, 0.0f), mean((size_t)n, 0.0f);
    dist[0] = 1.0f;
    size_t widest = 0;
    long total = 0, ties = 0;
    int last_t = 0;
    double lo = 1e9, hi = -1e9;
    for (int a = 1; a < n; ++a) {
        float* D = &dist[(size_t)a * kB1T];
        int choice[kBoRolls];
        for (int r = 0; r < kBoRolls; ++r) {
            int r0, r1;
            bo_roll(r, r0, r1);
            B1Argmin pick{mean.data(), index_of.data(), K, 0, 0, 0.0f};
            Collect set;
            auto both = [&](uint32_t pack, int l) { pick(pack, l); set(pack, l); };     // one walk feeds both
            bo_visit(cfg[a].pack, r0, r1, both);
            if (pick.len == 0 || pick.arg >= a) { fprintf(stderr, "no play from %x\n", cfg[a].pack); return 1; }
            choice[r] = pick.arg;
            set.finish();
            widest = std::max(widest, set.packs.size());
            total += (long)set.packs.size();
            int at_min = 0;
            for (uint32_t p : set.packs) at_min += mean[index_of[b1_rank(p, K)]] == pick.best;
            ties += at_min > 1;
        }
        for (int t = 1; t < kB1T; ++t) {
            float acc = 0.0f;
            int r = 0;
            for (int r0 = 1; r0 <= 6; ++r0)
                for (int r1 = r0; r1 <= 6; ++r1, ++r) {
                    const float p = r0 == r1 ? 1.0f / 36.0f : 2.0f / 36.0f;
                    const float prod = p * dist[(size_t)choice[r] * kB1T + t - 1];
                    acc = acc + prod;
                }
            D[t] = acc;
        }
        float m = 0.0f;
        double sum = 0.0;
        for (int t = 1; t < kB1T; ++t) {
            const float prod = (float)t * D[t];
            m = m + prod;
            sum += D[t];
            if (D[t] != 0.0f) last_t = std::max(last_t, t);
        }
        mean[a] = m;
        lo = std::min(lo, sum); hi = std::max(hi, sum);
    }
    auto mean_of_six_point = [&](int k) {
        const float v = mean[index_of[b1_rank((uint32_t)k << 20, K)]];
        uint32_t bits;
        memcpy(&bits, &v, 4);
        printf(" %.6f 0x%08x", v, bits);
    };
    printf("K %d n %d widest %zu total %ld ties %ld last_t %d rowsum %.9f %.9f means", K, n, widest, total, ties, last_t,
           lo, hi);
    mean_of_six_point(K < 6 ? K : 6);
    mean_of_six_point(K);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    const int K = argc > 2 ? atoi(argv[2]) : 0;
    if (argc < 3 || K < 1 || K > kB1MaxK) return 2;
    if (!strcmp(argv[1], "succ")) return run_succ(K);
    if (!strcmp(argv[1], "table")) return run_table(K);
    return 2;
}
