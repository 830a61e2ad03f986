// rtr_stamp_rule.h -- the tile store's 24-bit frame stamp (TileStore::seq, rtr_kernels.h): the next stamp of a store,
// whether its extent directory must be cleared first, and how many bytes that clear covers.  Host only and free of
// HIP (tests/cpp/stamp_rule_check.cpp compiles it with g++); next_seq() in rtr_api.hip is its one caller.
//
// A directory word is extent base << 24 | stamp and is current only while stamp == TileStore::seq, so a stamp must
// never come round again while a word that carries it is still in the directory: the frame that would take stamp 0
// clears the whole directory first and takes 1 instead.  0 is never a frame's stamp -- it is what a cleared word holds.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rtr {

constexpr uint32_t kStampMask = 0xFFFFFFu;  // 24 bits: the stamp shares an 8-byte directory word with a 40-bit base
constexpr int kDirK = 21;                   // directory words per storage tile: extents 1..20 reach 2^32 entries

struct StampStep {
    uint32_t stamp;  // the stamp of the frame about to be binned, 1 .. kStampMask
    bool clear;      // the directory must be cleared before that frame's point kernel runs
};

inline StampStep next_stamp(uint32_t cur) {
    const uint32_t next = (cur + 1u) & kStampMask;
    return next == 0u ? StampStep{1u, true} : StampStep{next, false};
}

// bytes of a store's directory: kDirK 8-byte words for each of its nst storage tiles
inline size_t dir_bytes(int nst) { return (size_t)nst * kDirK * sizeof(uint64_t); }

}  // namespace rtr
