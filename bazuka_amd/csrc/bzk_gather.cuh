// A gathered message: bytes that are not one range of memory, hashed in place (bzk_sha512.cuh and bzk_keccak.cuh absorb one; eddsa.hip's
// l1_tx_verify_kernel and l1_tx_hash_kernel build one per lane; the ctx = NULL entries run the same code).
//
// The signed form of an L1 `Transaction` (src/core/transaction.rs:369-397) is its bincode with the signature replaced by `Signature::Unsigned`
// and, for CreateContract / UpdateContract, with the optional state / delta in the middle of the record replaced by `None`:
//
//     rec[0 .. cut_a) | 00 | rec[cut_b .. sig_tag) | 00 00 00 00
//
// and Ed25519 hashes R | A in front of it.  Every inserted byte is zero, so a message is a short list of pieces, each either a range of the
// record or a run of zeros: at most six.  All ranges are ranges of one base pointer (R and A lie in the record too), so a piece is two 32-bit
// words: its offset from the base (ZEROS: a zero run) and the position in the message at which it ends.
//
// Bytes are fetched eight at a time where the eight lie inside one piece, byte by byte in a rolled loop at piece edges and past the end (bytes
// at or past the message's length read as zero: the hashes add their padding themselves).  SHA-512 reads its words big-endian, Keccak
// little-endian: fetch8_le is the word as it lies in memory, fetch8_be its byte swap.
#pragma once
#include "bzk_field.cuh"

namespace bzk {
namespace gather {

constexpr int MAX_PIECES = 6;
constexpr uint32_t ZEROS = 0xffffffffu;  // Msg::off of a zero run

struct Msg {
    const uint8_t* base;
    uint32_t off[MAX_PIECES];  // where the piece starts, from base; ZEROS for a zero run
    uint32_t end[MAX_PIECES];  // the position in the message at which the piece ends (non-decreasing; unused pieces repeat the total)
};

BZK_HD Msg msg_empty(const uint8_t* base) {
    Msg m;
    m.base = base;
#pragma unroll
    for (int k = 0; k < MAX_PIECES; ++k) {
        m.off[k] = ZEROS;
        m.end[k] = 0;
    }
    return m;
}
// piece K (pieces are set in order, K = 0 first): len bytes at base + off, or len zeros; the pieces after it are left empty.  K is a constant so
// that the two arrays stay in registers.
template <int K>
BZK_HD void set_piece(Msg& m, uint32_t off, uint32_t len) {
    const uint32_t e = (K ? m.end[K ? K - 1 : 0] : 0) + len;
    m.off[K] = off;
#pragma unroll
    for (int j = K; j < MAX_PIECES; ++j) m.end[j] = e;
}
BZK_HD uint64_t total(const Msg& m) { return m.end[MAX_PIECES - 1]; }

// The signed form of a record: rec[0 .. cut_a) | 00 | rec[cut_b .. sig_tag) | 00 00 00 00, or rec[0 .. sig_tag) | 00 00 00 00 where the record has
// no cut (cut_a == cut_b); WITH_RA: R | A (the 32 bytes at r_off, the 32 at a_off) in front, which is what Ed25519 hashes.  rec_off: the record's
// first byte from base; the other offsets are inside the record.  Always six slots, without a branch: what a form lacks is a piece of length 0.
template <bool WITH_RA>
BZK_HD Msg signed_form(const uint8_t* base, uint32_t rec_off, uint32_t cut_a, uint32_t cut_b, uint32_t sig_tag, uint32_t r_off, uint32_t a_off) {
    const bool cut = cut_a != cut_b;
    Msg m = msg_empty(base);
    set_piece<0>(m, rec_off + r_off, WITH_RA ? 32 : 0);
    set_piece<1>(m, rec_off + a_off, WITH_RA ? 32 : 0);
    set_piece<2>(m, rec_off, cut ? cut_a : sig_tag);
    set_piece<3>(m, ZEROS, cut ? 1 : 0);  // the None tag
    set_piece<4>(m, rec_off + cut_b, cut ? sig_tag - cut_b : 0);
    set_piece<5>(m, ZEROS, 4);  // Signature::Unsigned
    return m;
}

// The piece lookups below are chains of selects over constant indices, not early returns: a return from inside the unrolled loop lets the
// compiler merge the returns' loads into one with a variable index, which takes the two arrays out of registers.
//
// the byte at pos; 0 at or past the message's end
BZK_HD uint32_t byte_at(const Msg& m, uint64_t pos) {
    uint32_t start = 0, off = ZEROS, rel = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < MAX_PIECES; ++k) {
        const bool in = !found && pos < m.end[k];
        off = in ? m.off[k] : off;
        rel = in ? (uint32_t)pos - start : rel;
        found = found || in;
        start = m.end[k];
    }
    return off == ZEROS ? 0u : m.base[(uint64_t)off + rel];
}
// the eight bytes at pos .. pos + 8 as a little-endian word
BZK_HD uint64_t fetch8_le(const Msg& m, uint64_t pos) {
    uint32_t start = 0, off = ZEROS, rel = 0;
    bool whole = false;  // the eight bytes lie inside one piece
#pragma unroll
    for (int k = 0; k < MAX_PIECES; ++k) {
        const bool in = pos >= start && pos + 8 <= m.end[k];
        off = in ? m.off[k] : off;
        rel = in ? (uint32_t)pos - start : rel;
        whole = whole || in;
        start = m.end[k];
    }
    uint64_t w = 0;
    if (whole) {  // the fast path
        if (off != ZEROS) __builtin_memcpy(&w, m.base + (uint64_t)off + rel, 8);
        return w;
    }
    if (pos >= start) return 0;  // past the end
#pragma unroll 1
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte_at(m, pos + k) << (8 * k);  // rolled: piece edges are rare
    return w;
}
BZK_HD uint64_t fetch8_be(const Msg& m, uint64_t pos) { return __builtin_bswap64(fetch8_le(m, pos)); }

}  // namespace gather
}  // namespace bzk
