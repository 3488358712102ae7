// The staging loop of a host-pointer batch call: its records go through the call's workspace in rounds (bzk_rounds.h cut_rounds).  A call
// declares its columns once, in the order its buffers lie in the layout; run() then does, per round and in one stream, the uploads in that order,
// the caller's launches, the downloads in that order, and after the last round the overwrites of the registered secrets and one synchronise.
// Plain C++: the four device operations go through Dev (the product: bzk_internal.h StreamOps; tests/host/stage_check.hip: memcpy / memset).
#pragma once
#include <vector>

#include "../../include/bzk.h"
#include "bzk_rounds.h"
#include "bzk_ws.h"

namespace bzk {

// Dev: int32_t up(dev, host, bytes), down(host, dev, bytes), zero(dev, bytes), sync() - BZK_OK, or the status the call returns
template <class Dev>
struct Stage {
    Dev dev;
    WsLayout ws;                     // the call's one layout: the columns below and whatever else the caller takes; the caller commits it
    std::vector<uint64_t> round_at;  // cut_rounds' starts
    uint64_t cap = 0, cap_bytes = 0; // records and bytes of the byte column (off) in the longest round

    // rounds of at most max_records records and max_weight summed weight(i); off (n + 1 offsets, or null): what the byte column uploads
    template <class W>
    Stage(Dev d, const char* who, uint64_t n, uint64_t max_records, uint64_t max_weight, W weight, const uint64_t* off)
        : dev(d), ws(who), round_at(cut_rounds(n, max_records, max_weight, weight)), off_(off) {
        const RoundCaps rc = round_caps(round_at, off);
        cap = rc.cap;
        cap_bytes = rc.cap_bytes;
    }
    Stage(Dev d, const char* who, uint64_t n, uint64_t max_records)
        : Stage(d, who, n, max_records, ~(uint64_t)0, [](uint64_t) { return (uint64_t)0; }, nullptr) {}

    // Fixed-stride columns: a round of m records from a moves m * stride bytes between host + a * stride and the buffer.  `parts` columns may
    // share a buffer of cap * stride * parts bytes: in / out declare it and are its part 0, in_part / out_part move part k at p + k * m * stride.
    void in(uint8_t*& p, const void* host, size_t stride, size_t parts = 1) { ws.take(p, cap * stride * parts); in_part(p, host, stride, 0); }
    void in_part(uint8_t*& p, const void* host, size_t stride, size_t k) { cols_.push_back({FIXED, &p, (const uint8_t*)host, nullptr, stride, k}); }
    // a null host pointer: the buffer exists and nothing is copied back
    void out(uint8_t*& p, void* host, size_t stride, size_t parts = 1) { ws.take(p, cap * stride * parts); out_part(p, host, stride, 0); }
    void out_part(uint8_t*& p, void* host, size_t stride, size_t k) { cols_.push_back({FIXED, &p, nullptr, (uint8_t*)host, stride, k}); }
    void scratch(uint8_t*& p, size_t stride) { ws.take(p, cap * stride); }
    // the variable-length column, prefix + cap_bytes + pad bytes: a round uploads host[off[a] .. off[b]) behind the prefix (nothing where it is empty)
    void bytes(uint8_t*& p, const uint8_t* host, size_t prefix, size_t pad) {
        ws.take(p, prefix + cap_bytes + pad);
        cols_.push_back({BYTES, &p, host, nullptr, 0, prefix});
    }
    void offsets(uint8_t*& p) {  // off[a .. b], m + 1 entries as they stand (the kernels subtract off[a])
        ws.take(p, (cap + 1) * 8);
        cols_.push_back({OFFSETS, &p, nullptr, nullptr, 0, 0});
    }
    // the first `bytes` of a declared buffer held secrets: zero after the last round, and on every early way out of run()
    void wipe(uint8_t*& p, size_t bytes) { wipes_.push_back({&p, bytes}); }

    // launch(a, m): enqueue the kernels of the round [a, a + m); BZK_OK or the status to return
    template <class F>
    int32_t run(F&& launch) {
        struct Guard {  // the early way out: the same overwrites, their failure unreported
            Stage& s;
            bool armed = true;
            ~Guard() {
                if (!armed || s.wipes_.empty()) return;
                for (const Wipe& w : s.wipes_) (void)s.dev.zero(*w.p, w.bytes);
                (void)s.dev.sync();
            }
        } guard{*this};
        int32_t rc;
        for (size_t c = 0; c + 1 < round_at.size(); ++c) {  // one stream: a round's uploads follow the previous round's kernels
            const uint64_t a = round_at[c], m = round_at[c + 1] - a;
            for (const Col& k : cols_) {
                if (k.kind == BYTES && off_[a + m] != off_[a]) rc = dev.up(*k.p + k.part, k.up + off_[a], off_[a + m] - off_[a]);
                else if (k.kind == OFFSETS) rc = dev.up(*k.p, off_ + a, (m + 1) * 8);
                else if (k.kind == FIXED && k.up) rc = dev.up(*k.p + k.part * m * k.stride, k.up + a * k.stride, m * k.stride);
                else continue;
                if (rc != BZK_OK) return rc;
            }
            if ((rc = launch(a, m)) != BZK_OK) return rc;
            for (const Col& k : cols_)
                if (k.down && (rc = dev.down(k.down + a * k.stride, *k.p + k.part * m * k.stride, m * k.stride)) != BZK_OK) return rc;
        }
        for (const Wipe& w : wipes_)
            if ((rc = dev.zero(*w.p, w.bytes)) != BZK_OK) return rc;
        if ((rc = dev.sync()) != BZK_OK) return rc;
        guard.armed = false;
        return BZK_OK;
    }

private:
    enum Kind { FIXED, BYTES, OFFSETS };
    struct Col {
        Kind kind;
        uint8_t** p;
        const uint8_t* up;
        uint8_t* down;
        size_t stride, part;  // BYTES: part is the prefix
    };
    struct Wipe {
        uint8_t** p;
        size_t bytes;
    };
    const uint64_t* off_;
    std::vector<Col> cols_;
    std::vector<Wipe> wipes_;
};

}  // namespace bzk
