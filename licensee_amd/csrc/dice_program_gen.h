// Generator of the template-specialized sparse scoring program: plan_program() decides everything
// about a corpus's program, emit_program() writes its HIP source. Host C++ only, no HIP header: the
// sanitizer driver (tests/sanitize/program_driver.cpp) builds it with g++. dice_program.cpp compiles,
// loads and launches what is emitted here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/licensee_dice.h"

namespace dice {

constexpr int32_t kProgramWaves = 4;    // waves (64-file tiles) per workgroup (1, 2 and 8 within +-1.5%)
constexpr int kMaxIndexedTemplates = 255;   // the match kernels keep the template index in one byte, 0xFF = none yet
constexpr int kMfmaMatchWaves = 12;     // MWK of the generated matrix-core match kernel

// What the environment may choose (program_options_from_env in dice_program.cpp reads it, at
// dice_create and in the exports; nothing below reads the environment).
struct ProgramOptions {
    enum Match { kAuto, kValu, kMfma };
    enum Diag { kNone, kNoAcc, kNoEpi, kTiming, kNoMfma };
    bool compact = true;    // DICE_PROG_LAYOUT: class-count tile, or (`bits`) the full-bitset tile
    Match match = kAuto;    // DICE_PROG_MATCH: `mfma` takes the matrix-core stage wherever it is eligible,
                            // `valu` never; by default the cost rule decides
    Diag diag = kNone;      // DICE_PROG_DIAG, -DDICE_DIAG builds only: results are wrong
    // quads per load group: 5 for both tiles (3, 4, 5 and 7 measure alike on the compact tile's 14 quads)
    int burst = 5;
};

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

// The order the program runs in. Tile slot i holds quad qperm[i] of the layout (of the vocabulary,
// full-bitset tile) and is processed i-th, so a wave's loads walk its tile front to back.
struct Schedule {
    std::vector<Entry> dm;                            // the entries sorted by (dword, tpl)
    std::vector<std::pair<size_t, size_t>> range;     // per processed slot: its entries [begin, end) in dm
    std::vector<int32_t> qperm;                       // [tile quads]: the processed slots, then the quads no template reads
};

// One piece of a compact tile dword (the generated dice_pack_compact): v = row_dword[src] & mask
// contributes v << op (0 <= op < 32), v >> -op (op < 0) or popcount(v) << (op - 64) (op >= 64).
struct PackPiece {
    int32_t src;
    uint32_t mask;
    int32_t op;
};

// Tables of the matrix-core accumulate stage over the compact tile's bit region (kMfmaPrelude in
// dice_program_gen.cpp). K-step s takes, per lane half h, one tile dword: dword s % 4 of
// the quad in slot slots[2 (s / 4) + h] (-1: none, the template elements are zero). The device
// holds the templates in the rows assign_rows chose (rows[], two blocks of 32): with the bit region
// grouped by block (group_bits) many (K-step, block) fragments are all zero, and the kernel neither
// reads nor multiplies those (live[]).
struct MfmaTables {
    int32_t ksteps = 0;               // K-steps of 64 elements (4 per pair of bit quads)
    int32_t ntiles = 0;               // 32-template tiles
    std::vector<int32_t> slots;       // [ksteps / 2] tile slot of the quad each lane half loads (-1: padding)
    std::vector<uint32_t> frag;       // [ksteps][ntiles][64][4] pre-widened template fragments, row 32 j + r = template 32 j + r
    std::vector<int32_t> map;         // [ksteps][64] tile bit carried by element e of half h (at 32 h + e), or -1
    std::vector<int32_t> rows;        // [32 ntiles] template in device row 32 j + r, or -1 (padding)
    std::vector<uint8_t> live;        // [ksteps][ntiles] 1: the fragment of device block j has a non-zero element
    std::vector<uint32_t> dfrag;      // frag with its rows gathered through rows[]: the device table dice_mfma_frag
    int32_t n_live = 0;               // fragments the kernel reads and multiplies
    int64_t valu_cost = 0;            // VALU instructions of the bit entries the stage replaces
    int64_t stage_cost = 0;           // the stage in VALU-issue units: fixed VALU + matrix cycles / 4
    bool eligible = false;            // a bit region, and the fragments fit in LDS at >= 2 waves per SIMD
    bool pays = false;                // cost rule (kMfmaPayRatio)
};

struct Program {
    ProgramOptions opts;
    int32_t wq = 0;                   // quads of the file tile the kernels read
    CompactLayout layout;             // compact tile only
    std::vector<Entry> prog;          // template-major, dword ascending
    Schedule sched;
    MfmaTables mf;                    // compact tile only; frag and map where mf.eligible
    bool mfma = false;                // the module also holds dice_prog_match_mfma
    bool mfma_forced = false;         // DICE_PROG_MATCH=mfma: small batches take it too
    std::vector<std::vector<PackPiece>> pack_lists;   // compact tile: [4 * quads] pieces per tile dword (slot order)
};

// Everything about the corpus's program but its text. A pure function of its arguments.
Program plan_program(const dice_templates* t, const ProgramOptions& opts);
// The HIP source of a planned program: five kernels, and dice_pack_compact for the compact tile.
std::string emit_program(const dice_templates* t, const Program& p);

}  // namespace dice
