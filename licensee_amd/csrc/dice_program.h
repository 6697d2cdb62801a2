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

// Tables of the matrix-core accumulate stage over the compact tile's bit region (dice_program.cpp,
// "Matrix-core accumulate stage"). K-step s takes, per lane half h, one tile dword: dword s % 4 of
// the quad in slot slots[2 (s / 4) + h] (-1: none, the template elements are zero).
struct MfmaTables {
    int32_t ksteps = 0;               // K-steps of 64 elements (4 per pair of bit quads)
    int32_t ntiles = 0;               // 32-template tiles
    std::vector<int32_t> slots;       // [ksteps / 2] tile slot of the quad each lane half loads (-1: padding)
    std::vector<uint32_t> frag;       // [ksteps][ntiles][64][4] pre-widened template fragments
    std::vector<int32_t> map;         // [ksteps][64] tile bit carried by element e of half h (at 32 h + e), or -1
    int64_t valu_cost = 0;            // VALU instructions of the bit entries the stage replaces
    int64_t stage_cost = 0;           // the stage in VALU-issue units: fixed VALU + matrix cycles / 4
    bool eligible = false;            // a bit region, and the fragments fit in LDS at >= 2 waves per SIMD
    bool pays = false;                // cost rule (kMfmaPayRatio)
};

struct Program {
    bool mfma = false;                // the module also holds dice_prog_match_mfma
    bool mfma_forced = false;         // DICE_PROG_MATCH=mfma: small batches take them too
    MfmaTables mf;
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
