// Host check of the search workspaces' layouts (csrc/bg_workspace.h): built with
// -fsanitize=address,undefined and run by tests/test_search_workspace_cpu.py.
#include <stdio.h>
#include <vector>

#include "bg_workspace.h"

using namespace bgws;

struct Span { const char* name; size_t off, bytes; };
template <typename T>
static Span span(const char* name, const Region<T>& r) { return {name, r.off, r.bytes()}; }

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// regions in declaration order: each on a 256-byte boundary, none before the end of the
// one before it, all at or after `start`, and `total` the aligned end of the last
static void check_regions(const char* what, const std::vector<Span>& regions, size_t start, size_t total) {
    size_t end = start;
    for (const Span& s : regions) {
        EXPECT(s.off % 256 == 0, "%s.%s at %zu", what, s.name, s.off);
        EXPECT(s.off >= end, "%s.%s at %zu overlaps the region before it (ends %zu)", what, s.name, s.off, end);
        end = s.off + s.bytes;
    }
    EXPECT(total == align_up(end), "%s: bytes() %zu, last region ends %zu", what, total, end);
    EXPECT(total % 256 == 0, "%s: bytes() %zu", what, total);
}

static void check_one_ply(size_t B, size_t M, bool with_kept) {
    const OnePlyLayout L(B, M, with_kept);
    const size_t R = B * M;
    std::vector<Span> r = {span("lane_off", L.lane_off), span("total", L.total), span("row_lane", L.row_lane),
                           span("rowside", L.rowside), span("rowkey", L.rowkey), span("vrow", L.vrow)};
    if (with_kept) {
        r.push_back(span("kept", L.kept));
        r.push_back(span("kept_move", L.kept_move));
    }
    check_regions("one_ply", r, 0, L.bytes());
    EXPECT(L.lane_off.off == 0 && L.lane_off.count == B && L.total.count == 1, "B %zu", B);
    EXPECT(L.row_lane.count == R && L.rowside.count == R && L.rowkey.count == R && L.vrow.count == R, "R %zu", R);
    EXPECT(!with_kept || (L.kept.count == B && L.kept_move.count == R), "B %zu R %zu", B, R);
    // the filter's regions come after the plain ones: the plain pass's regions do not move
    const OnePlyLayout P(B, M, false);
    EXPECT(P.vrow.off == L.vrow.off && P.bytes() <= L.bytes(), "B %zu M %zu", B, M);
}

static void check_two_ply(size_t B, size_t rows, int NT, bool filtered) {
    const size_t jobs = rows * 21;
    const TwoPlyLayout H(B);
    EXPECT(H.bytes() == H.head_bytes(), "B %zu", B);
    check_regions("two_ply head", {span("lane_off", H.lane_off), span("ctr", H.ctr), span("queues", H.queues)}, 0,
                  H.head_bytes());
    EXPECT(H.ctr.bytes() <= 256 && H.queues.off == H.ctr.off + 256, "counter block");
    TwoPlyLayout L(B);
    L.body(rows, jobs, NT, filtered);
    // the head does not depend on the body (a regrow keeps it by copying head_bytes())
    EXPECT(L.lane_off.off == H.lane_off.off && L.ctr.off == H.ctr.off && L.queues.off == H.queues.off &&
           L.head_bytes() == H.head_bytes(), "B %zu rows %zu NT %d", B, rows, NT);
    std::vector<Span> r = {span("row_lane", L.row_lane), span("rowrec", L.rowrec), span("rowside", L.rowside),
                           span("minv", L.minv), span("maxlen", L.maxlen), span("list", L.list),
                           span("retry", L.retry), span("rowpart", L.rowpart)};
    if (filtered) r.push_back(span("row_move", L.row_move));
    check_regions("two_ply body", r, L.head_bytes(), L.bytes());
    EXPECT(L.row_lane.off == L.head_bytes(), "body starts at the head's end");
    EXPECT(L.row_lane.count == rows && L.rowrec.bytes() == rows * 64 && L.rowside.bytes() == rows * 16, "rows %zu", rows);
    EXPECT(L.minv.count == jobs && L.maxlen.count == jobs && L.list.count == jobs && L.retry.count == jobs, "jobs %zu",
           jobs);
    EXPECT(L.rowpart.count == rows * 16 * (size_t)(NT <= 4 ? NT : (NT + 1) / 2 * 2), "rows %zu NT %d", rows, NT);
    EXPECT(!filtered || L.row_move.count == rows, "rows %zu", rows);
    // body() again with other sizes starts over from the head
    L.body(rows + 1, jobs + 21, NT, filtered);
    L.body(rows, jobs, NT, filtered);
    EXPECT(L.row_lane.off == L.head_bytes() && L.bytes() == (r.back().off + r.back().bytes + 255) / 256 * 256, "re-body");
}

int main() {
    for (size_t B : {1, 3, 64, 256, 4096, 65536})
        for (size_t M : {1, 7, 500})
            for (int k = 0; k < 2; ++k) check_one_ply(B, M, k != 0);
    // rows: none, one, odd, the filter test's, the benchmark's, the most whose jobs fit 29-bit tags
    const size_t kMostRows = (0x1FFFFFFF - 1) / 21;
    static_assert(kMostRows * 21 < 0x1FFFFFFF && (kMostRows + 1) * 21 >= 0x1FFFFFFF, "29-bit job tags");
    for (size_t B : {1, 3, 64, 256, 65536})
        for (size_t rows : {(size_t)0, (size_t)1, (size_t)63, (size_t)5000, (size_t)1300000, kMostRows})
            for (int NT = 1; NT <= 8; ++NT)
                for (int f = 0; f < 2; ++f) check_two_ply(B, rows, NT, f != 0);
    // the memory footprint, from the expressions the layouts replaced
    EXPECT(OnePlyLayout(4096, 500, false).bytes() == 81936640u, "%zu", OnePlyLayout(4096, 500, false).bytes());
    EXPECT(OnePlyLayout(4096, 500, true).bytes() == 90145024u, "%zu", OnePlyLayout(4096, 500, true).bytes());
    TwoPlyLayout L(256);
    L.body(5000, 105000, 3, true);
    EXPECT(L.head_bytes() == 12584192u && L.bytes() == 15350272u, "%zu %zu", L.head_bytes(), L.bytes());
    static_assert(sizeof(Ctr) <= 256, "the counter block");
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("workspace ok\n");
    return 0;
}
