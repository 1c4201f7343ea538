// bg_workspace.h — the byte layouts of bg_search.hip's device workspaces.
// Each pass describes its workspace once, as a layout: the layout gives the size to
// reserve and, from the buffer's base pointer, every typed region.  Plain C++17, no HIP:
// tests/cpp/workspace_main.cpp checks the layouts on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bgws {

constexpr size_t kAlign = 256;
constexpr size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

// a 16-byte element where HIP's uint4 is not at hand (read it as one: at<uint4>)
struct alignas(16) Vec16 { uint32_t x, y, z, w; };

// `count` elements of T at byte `off` of a workspace
template <typename T>
struct Region {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    template <typename U = T>
    U* at(void* base) const {
        static_assert(sizeof(U) == sizeof(T), "a region is read with its own element size");
        return (U*)((char*)base + off);
    }
};

// Bump carver over a byte range: every region starts on a 256-byte boundary.
class Carver {
    size_t top_;
public:
    explicit Carver(size_t start = 0) : top_(start) {}
    template <typename T>
    Region<T> take(size_t count) {
        const Region<T> r{top_, count};
        top_ = align_up(top_ + r.bytes());
        return r;
    }
    size_t bytes() const { return top_; }
};

// 1-ply rows, sized for the worst case (B x max_moves rows) so that the pass runs without
// a host sync: the row count stays on the device.  with_kept: room for the move filter's
// kept counts and kept move lists after them.
struct OnePlyLayout {
    Region<int32_t> lane_off;      // [B] first row of each lane
    Region<int64_t> total;         // the row count
    Region<int32_t> row_lane;      // [R]
    Region<Vec16> rowside, rowkey; // [R] each
    Region<float> vrow;            // [R] V per row
    Region<int32_t> kept;          // [B], with_kept only
    Region<int32_t> kept_move;     // [R], with_kept only
    bool with_kept;
    OnePlyLayout(size_t B, size_t max_moves, bool with_kept_) : with_kept(with_kept_) {
        const size_t R = B * max_moves;
        lane_off = c_.take<int32_t>(B);
        total = c_.take<int64_t>(1);
        row_lane = c_.take<int32_t>(R);
        rowside = c_.take<Vec16>(R);
        rowkey = c_.take<Vec16>(R);
        vrow = c_.take<float>(R);
        if (with_kept) {
            kept = c_.take<int32_t>(B);
            kept_move = c_.take<int32_t>(R);
        }
    }
    size_t bytes() const { return c_.bytes(); }
private:
    Carver c_;
};

// the 2-ply pass's counters: one 256-byte block in the workspace head, zeroed per call
struct Ctr {
    int64_t rows;
    unsigned long long leaves, cursor;
    int32_t qcount[3], retry_count, list_count, bad;    // bad: k_rows found a changed lane
    unsigned long long zero;                            // start of the evaluated pool range
};
static_assert(sizeof(Ctr) <= 256, "counters");

constexpr int kSlowQueue = 1 << 20;      // jobs per overflow queue
// 16-unit slices of the packed value net: the wide form (NT > 4) pads to whole 32-unit tiles
constexpr bool wide_tiles(int NT) { return NT > 4; }
constexpr int slices(int NT) { return wide_tiles(NT) ? (NT + 1) & ~1 : NT; }

// 2-ply workspace, in two steps: the head is needed to count the rows, the body is sized by
// that count.  The head's offsets depend on B alone, so a regrow between the two steps
// keeps the head by copying its bytes.
struct TwoPlyLayout {
    // head
    Region<int32_t> lane_off;      // [B]
    Region<Ctr> ctr;
    Region<int32_t> queues;        // [3][kSlowQueue] overflow queues
    // body
    Region<int32_t> row_lane;      // [rows]
    Region<uint8_t> rowrec;        // [rows][64]
    Region<Vec16> rowside;         // [rows]
    Region<int32_t> minv;          // [jobs]
    Region<uint8_t> maxlen;        // [jobs]
    Region<int32_t> list, retry;   // [jobs] each
    Region<float> rowpart;         // [rows][16 * slices(NT)]
    Region<int32_t> row_move;      // [rows], filtered only
    bool filtered = false;
    explicit TwoPlyLayout(size_t B) {
        Carver c;
        lane_off = c.take<int32_t>(B);
        ctr = c.take<Ctr>(1);
        queues = c.take<int32_t>((size_t)3 * kSlowQueue);
        head_ = total_ = c.bytes();
    }
    void body(size_t rows, size_t jobs, int NT, bool filtered_) {
        Carver c(head_);
        filtered = filtered_;
        row_lane = c.take<int32_t>(rows);
        rowrec = c.take<uint8_t>(rows * 64);
        rowside = c.take<Vec16>(rows);
        minv = c.take<int32_t>(jobs);
        maxlen = c.take<uint8_t>(jobs);
        list = c.take<int32_t>(jobs);
        retry = c.take<int32_t>(jobs);
        rowpart = c.take<float>(rows * 16 * (size_t)slices(NT));
        if (filtered) row_move = c.take<int32_t>(rows);
        total_ = c.bytes();
    }
    size_t head_bytes() const { return head_; }
    size_t bytes() const { return total_; }     // head alone until body() has run
private:
    size_t head_, total_;
};

// bgx_roll_luck's additions to the 2-ply workspace, behind the TwoPlyLayout of the same call
// (start = its bytes() after body()): the luck form of the value pack, derived per call.
// The TwoPlyLayout regions keep their offsets; the head stays the part kept over a regrow.
struct LuckLayout {
    Region<float> pack;            // [pack_floats] luck form of the bgx_value_pack pack
    LuckLayout(size_t start, size_t pack_floats) {
        Carver c(align_up(start));
        start_ = c.bytes();
        pack = c.take<float>(pack_floats);
        total_ = c.bytes();
    }
    size_t start() const { return start_; }
    size_t bytes() const { return total_; }     // end of the whole workspace (2-ply part included)
private:
    size_t start_, total_;
};

}  // namespace bgws
