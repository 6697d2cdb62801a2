// Template-specialized sparse scoring program (declarations). See dice_program.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/licensee_dice.h"

namespace dice {

// One program entry: accumulate popcount(file_dword[dword] & mask) into template `tpl`; with
// `sum` (a count dword of the compact tile) the sum of the dword's bytes selected by `mask`.
struct Entry {
    int32_t tpl;
    int32_t dword;
    uint32_t mask;
    bool sum = false;
};

// Compact tile layout (class-count tile): vocabulary words that belong to exactly the same set
// of templates are interchangeable for every overlap, so a class of more than `threshold` such
// words is stored as byte counts (fields of capacity <= 255) instead of bits. The tile holds
// the bit region (the caller's vocabulary order with count-class and unused words removed),
// then the count bytes. A pure function of dice_templates.
struct CompactLayout {
    int32_t threshold = 0;        // classes of more words than this are count fields
    int32_t n_bits = 0;           // words kept as bits
    int32_t bit_dwords = 0;       // dwords of the bit region; count byte f is tile byte 4 * bit_dwords + f
    int32_t n_fields = 0;         // count bytes
    int32_t quads = 0;            // tile quads (16 B each per file)
    std::vector<int32_t> dest;    // per word: bit position (>= 0), -1 none, -2 - f count byte f
    std::vector<uint64_t> field_col;   // per count byte: its class's template set (bit i: template i)
};

// One piece of a compact tile dword (the generated dice_pack_compact): v = row_dword[src] & mask
// contributes v << op (0 <= op < 32), v >> -op (op < 0) or popcount(v) << (op - 64) (op >= 64).
struct PackPiece {
    int32_t src;
    uint32_t mask;
    int32_t op;
};

struct Program {
    std::vector<Entry> prog;          // sorted by (dword, tpl)
    std::vector<int32_t> dword_map;   // vocab dword -> file dword in the remapped layout (-1: unused)
    int32_t wpb = 4;                  // waves (64-file tiles) per workgroup
    std::vector<int32_t> qperm;       // tile slot -> vocabulary quad (empty: identity)
    bool compact = false;             // compact tile: qperm is tile slot -> layout quad
    CompactLayout layout;
    std::vector<std::vector<PackPiece>> pack_lists;   // [4 * quads] pieces per tile dword (slot order)
    size_t entries() const { return prog.size(); }
};

int program_setup(dice_ctx* c, const dice_templates* t);
// compact tile: b->d_rows[0, n) -> b->d_tiles
int program_launch_pack(dice_ctx* c, dice_batch* b, int64_t n, hipStream_t s);
int program_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s);
int program_launch_matrix(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s);

}  // namespace dice
