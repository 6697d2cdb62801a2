// Generator of the template-specialized sparse scoring program for small corpora (T <= 64), gfx950.
//
// The corpus is known when dice_create() runs, so the overlap loop
//     ov_t = sum_d popcount(file[d] & Lf_t[d])          (content_helper.rb:129)
// is emitted as straight-line HIP over the NONZERO (template, dword) pairs only: every file
// dword lives in a VGPR with a compile-time index and every template mask is an instruction
// literal, so an entry costs v_and_b32 (literal) + v_bcnt_u32_b32 (accumulate) and no
// memory traffic beyond the file's own bitset. With the interner's signature vocabulary
// order the 47 vendored templates need ~1.5k entries instead of 47 x 112 dense dwords,
// which moves the kernel from VALU-bound to HBM-bound.
//
// Each template's epilogue follows its accumulation: denominator
// (content_helper.rb:130-132,337-347, per-template constants baked in), CC filter
// (dice.rb:23-31) and the running argmax (dice.rb:34-48). The compare is an exact
// rational cross-multiplication on the fast path; waves holding a file outside the fast
// envelope (|W_F| >= 2^20 or len_F >= 2^21, or a corpus outside the envelope) run the same
// program with IEEE-double compares (see dice_common.h for why both orders coincide).
//
// By default the program runs over the compact tile (derive_layout below):
// words that belong to exactly the same templates are interchangeable for every overlap, so a
// large class of them is a byte count (one v_dot4_u32_u8 per template and count dword) instead of bits, and the
// file's tile is half as long. ProgramOptions::compact = false keeps the full-bitset tile. Where it
// pays (plan_mfma), the module also holds the match kernel with the bit region scored on the matrix
// cores (kMfmaPrelude); ProgramOptions::match overrides the rule.
//
// Two stages: plan_program (layout -> matrix-core shape, row assignment and word grouping -> entries
// -> schedule -> matrix-core tables and cost rule -> pack lists, no text) and emit_program (text from
// the plan, nothing else).
#include "dice_program_gen.h"

#include <algorithm>
#include <sstream>

namespace dice {

namespace {

// ---------------------------------------------------------------------------------------
// Plan
// ---------------------------------------------------------------------------------------

// The full-bitset tile's entry list (template-major, dword ascending) from the template bitsets.
std::vector<Entry> build_entries(const dice_templates* t, int32_t w64) {
    std::vector<Entry> out;
    const int32_t w32 = w64 * 2;
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(t->lf_bits + (size_t)i * w64);
        for (int32_t d = 0; d < w32; ++d)
            if (row[d]) out.push_back(Entry{i, d, row[d]});
    }
    return out;
}

// Template-membership column of every vocabulary word (bit i: the word is in template i).
std::vector<uint64_t> word_columns(const dice_templates* t) {
    const int32_t V = t->n_vocab, w64 = (V + 63) / 64;
    std::vector<uint64_t> col((size_t)V, 0);
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const uint64_t* row = t->lf_bits + (size_t)i * w64;
        for (int32_t v = 0; v < V; ++v)
            if ((row[v >> 6] >> (v & 63)) & 1) col[(size_t)v] |= 1ull << i;
    }
    return col;
}

struct WordClass {
    uint64_t col;
    std::vector<int32_t> words;   // ascending
};

// Places every word for class-size threshold `th`: classes of more than th words become count
// fields (capacity <= 255, the class's words split evenly in vocabulary order), the other words
// of some template keep a bit, in vocabulary order. Count fields are grouped four to a dword
// greedily by template set: a dword starts with the widest remaining set and takes the fields
// that add the fewest templates to it, so one masked byte sum serves several fields.
void place_words(const std::vector<WordClass>& classes, int32_t V, int32_t th, CompactLayout& L) {
    L.threshold = th;
    L.dest.assign((size_t)V, -1);
    struct Field {
        uint64_t col;
        std::vector<int32_t> words;
    };
    std::vector<Field> raw;
    std::vector<char> bit((size_t)V, 0);
    for (const WordClass& c : classes) {
        const int32_t sz = (int32_t)c.words.size();
        if (sz <= th) {
            for (int32_t v : c.words) bit[(size_t)v] = 1;
            continue;
        }
        const int32_t nf = (sz + 254) / 255, cap = (sz + nf - 1) / nf;
        for (int32_t f = 0; f < nf; ++f) {
            Field fd{c.col, {}};
            for (int32_t j = f * cap; j < std::min(sz, (f + 1) * cap); ++j) fd.words.push_back(c.words[(size_t)j]);
            raw.push_back(std::move(fd));
        }
    }
    L.n_bits = 0;
    for (int32_t v = 0; v < V; ++v)
        if (bit[(size_t)v]) L.dest[(size_t)v] = L.n_bits++;
    L.bit_dwords = (L.n_bits + 31) / 32;
    L.n_fields = (int32_t)raw.size();
    L.field_col.clear();
    std::vector<char> used(raw.size(), 0);
    auto pc = [](uint64_t x) { return __builtin_popcountll(x); };
    for (size_t placed = 0; placed < raw.size();) {
        uint64_t un = 0;
        for (int k = 0; k < 4 && placed < raw.size(); ++k, ++placed) {
            size_t pick = raw.size();
            for (size_t i = 0; i < raw.size(); ++i) {
                if (used[i]) continue;
                if (pick == raw.size()) { pick = i; continue; }
                const bool better = k == 0 ? pc(raw[i].col) > pc(raw[pick].col)
                                           : pc(un | raw[i].col) < pc(un | raw[pick].col);
                if (better) pick = i;
            }
            used[pick] = 1;
            un |= raw[pick].col;
            const int32_t f = (int32_t)L.field_col.size();
            L.field_col.push_back(raw[pick].col);
            for (int32_t v : raw[pick].words) L.dest[(size_t)v] = -2 - f;
        }
    }
    const int32_t dwords = L.bit_dwords + (L.n_fields + 3) / 4;
    L.quads = std::max(1, (dwords + 3) / 4);
}

// The compact tile's entry list (template-major, dword ascending).
void build_compact_entries(const dice_templates* t, const std::vector<uint64_t>& col, const CompactLayout& L,
                           std::vector<Entry>& out) {
    out.clear();
    const int32_t nd = L.bit_dwords + (L.n_fields + 3) / 4;
    std::vector<uint32_t> m((size_t)nd);
    for (int32_t i = 0; i < t->n_templates; ++i) {
        std::fill(m.begin(), m.end(), 0u);
        for (int32_t v = 0; v < t->n_vocab; ++v) {
            const int32_t p = L.dest[(size_t)v];
            if (p >= 0 && ((col[(size_t)v] >> i) & 1)) m[(size_t)(p >> 5)] |= 1u << (p & 31);
        }
        for (int32_t f = 0; f < L.n_fields; ++f)
            if ((L.field_col[(size_t)f] >> i) & 1) m[(size_t)(L.bit_dwords + f / 4)] |= 0xFFu << (8 * (f % 4));
        for (int32_t d = 0; d < nd; ++d)
            if (m[(size_t)d]) out.push_back(Entry{i, d, m[(size_t)d], d >= L.bit_dwords});
    }
}

// VALU instructions of an entry: v_and_b32 (not for a full mask) + v_bcnt_u32_b32. A count dword's
// entry is one v_dot4_u32_u8 now but keeps the weight it had as v_and_b32 + v_sad_u8: the layout
// choice and the slot order rest on these weights and stay what they were.
int entry_cost(const Entry& e) { return e.mask == 0xFFFFFFFFu ? 1 : 2; }

// Layout for the corpus and its entries: the class-size threshold that gives the fewest tile quads,
// on a tie the fewest program instructions (then the smallest threshold). A class of <= 8 words
// never takes more bits as bits than as a count byte, so thresholds start at 8. `col` is word_columns(t).
void derive_layout(const dice_templates* t, const std::vector<uint64_t>& col, CompactLayout& best, std::vector<Entry>& entries) {
    const int32_t V = t->n_vocab;
    std::vector<WordClass> classes;
    {
        std::vector<int32_t> order;
        for (int32_t v = 0; v < V; ++v)
            if (col[(size_t)v]) order.push_back(v);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return col[(size_t)a] < col[(size_t)b]; });
        for (int32_t v : order) {
            if (classes.empty() || classes.back().col != col[(size_t)v]) classes.push_back(WordClass{col[(size_t)v], {}});
            classes.back().words.push_back(v);
        }
    }
    std::vector<int32_t> ths{8};
    for (const WordClass& c : classes)
        if (c.words.size() > 8) ths.push_back((int32_t)c.words.size());
    std::sort(ths.begin(), ths.end());
    ths.erase(std::unique(ths.begin(), ths.end()), ths.end());
    int64_t best_cost = 0;
    bool have = false;
    for (int32_t th : ths) {
        CompactLayout L;
        std::vector<Entry> es;
        place_words(classes, V, th, L);
        build_compact_entries(t, col, L, es);
        int64_t cost = 0;
        for (const Entry& e : es) cost += entry_cost(e);
        if (!have || L.quads < best.quads || (L.quads == best.quads && cost < best_cost)) {
            best = std::move(L);
            entries.swap(es);
            best_cost = cost;
            have = true;
        }
    }
}

// Program order: dword-major -- every template accumulator stays live (acc[NT]); file quads are
// loaded in bursts right before they are consumed, so a file dword's live range is a few
// instructions; the epilogue (denominator, compare) runs once per template after the last quad.
// (The template-major order, the whole bitset loaded up front and each template retired in turn,
// measured 2% slower and is retired: DESIGN.md Appendix B.)
Schedule build_schedule(const std::vector<Entry>& entries, int32_t wq) {
    Schedule sc;
    sc.dm = entries;
    std::stable_sort(sc.dm.begin(), sc.dm.end(), [](const Entry& x, const Entry& y) {
        return x.dword != y.dword ? x.dword < y.dword : x.tpl < y.tpl;
    });
    // quads the program touches, their entry ranges in dm and their VALU cost
    std::vector<int32_t> quads;
    std::vector<std::pair<size_t, size_t>> range;
    std::vector<int> cost;
    for (size_t i = 0; i < sc.dm.size(); ++i) {
        if (quads.empty() || quads.back() != sc.dm[i].dword / 4) {
            quads.push_back(sc.dm[i].dword / 4);
            range.push_back({i, i});
            cost.push_back(0);
        }
        range.back().second = i + 1;
        cost.back() += entry_cost(sc.dm[i]);
    }
    // processing order: alternating costliest and cheapest quads, which spreads the VALU
    // work evenly over the stream (the packed vocabulary puts the widely shared words --
    // 120-250 VALU per quad -- at the end, the rare ones at 4-40 first): -5.5% config 2 vs
    // memory order (costliest-first -4.4%, equal VALU per burst +-0)
    std::vector<size_t> idx(quads.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
    std::vector<size_t> zip;
    for (size_t lo = 0, hi = idx.size(); lo < hi;) {
        zip.push_back(idx[lo++]);
        if (lo < hi) zip.push_back(idx[--hi]);
    }
    // Tile layout in processing order: tile slot i holds the quad processed i-th (dice_pack_tiles
    // and dice_pack_compact apply qperm), so a wave's loads walk its tile front to back while the
    // VALU work stays zipped.
    std::vector<char> seen((size_t)wq, 0);
    for (size_t i : zip) {
        sc.range.push_back(range[i]);
        sc.qperm.push_back(quads[i]);
        seen[(size_t)quads[i]] = 1;
    }
    for (int32_t q = 0; q < wq; ++q)
        if (!seen[(size_t)q]) sc.qperm.push_back(q);   // quads no template reads (never loaded)
    return sc;
}

// Cost rule of the matrix-core stage: it runs when the VALU instructions of the bit entries exceed
// kMfmaPayRatio times the stage's own cost in the same unit (one VALU issue = 4 cycles: widening 5
// per fragment, ~3 per template to fold, matrix cycles / 4 of the live fragments only). One measured
// point: the vendored corpus, ratio 2.02 with all 48 fragments multiplied, gained 1.21x (DESIGN.md
// section 4); with its 29 live ones the ratio is 2.74. The constant sits halfway between break-even
// on paper and the first point; it is not calibrated on a second corpus.
constexpr double kMfmaPayRatio = 1.5;
constexpr int64_t kMfmaMaxFragBytes = 96 * 1024;   // one 12-wave workgroup per CU: 3 waves per SIMD

// Shape of the stage for a layout (no word or slot order needed).
void plan_mfma(const dice_templates* t, const CompactLayout& L, MfmaTables& m) {
    const int32_t qb = (L.bit_dwords + 3) / 4, np = (qb + 1) / 2;
    m.ksteps = 4 * np;
    m.ntiles = (t->n_templates + 31) / 32;
    m.eligible = L.bit_dwords > 0 && (int64_t)m.ksteps * m.ntiles * 1024 <= kMfmaMaxFragBytes;
    m.rows.assign((size_t)32 * m.ntiles, -1);
    for (int32_t i = 0; i < t->n_templates; ++i) m.rows[(size_t)i] = i;
}

// Costs of the stage once its tables stand: only live fragments take matrix cycles.
void cost_mfma(const dice_templates* t, const std::vector<Entry>& entries, MfmaTables& m) {
    m.valu_cost = 0;
    for (const Entry& e : entries)
        if (!e.sum) m.valu_cost += entry_cost(e);
    const int64_t frags = m.eligible ? m.n_live : (int64_t)m.ksteps * m.ntiles;
    m.stage_cost = 2 * 5 * (int64_t)m.ksteps + 3 * (int64_t)t->n_templates + frags * 2 * 32 / 4;
    m.pays = m.eligible && (double)m.valu_cost > kMfmaPayRatio * (double)m.stage_cost;
}

// The bit region's dwords in K-step order: K-step s multiplies dwords 8 (s / 4) + s % 4 (lane half 0)
// and that + 4 (half 1), so a run of words laid along this sequence touches the fewest K-steps. The
// last pair of quads may be short: its K-steps then carry 32 elements, or none. ks_of[i] is the
// K-step of the i-th dword of the sequence (non-decreasing).
std::vector<int32_t> kstep_dwords(int32_t bit_dwords, int32_t ksteps, std::vector<int32_t>& ks_of) {
    std::vector<int32_t> seq;
    ks_of.clear();
    for (int32_t s = 0; s < ksteps; ++s)
        for (int32_t h = 0; h < 2; ++h) {
            const int32_t dw = 8 * (s / 4) + 4 * h + s % 4;
            if (dw >= bit_dwords) continue;
            seq.push_back(dw);
            ks_of.push_back(s);
        }
    return seq;
}

// Live fragments of the grouped bit region [a words of block 0 only | both | b of block 1 only] laid
// along kstep_dwords: block 0 is live on the K-steps of [0, a + both), block 1 on those of
// [a, a + both + b). Padding rule: the bit region has `slack` = 32 bit_dwords - n_bits unused bits,
// and 0 <= pad <= slack of them may follow the first group, which starts block 1 on a later K-step
// at the price of ending both blocks later; the smallest pad with the fewest live fragments is taken.
int32_t live_fragments(int32_t a, int32_t both, int32_t b, int32_t slack, const std::vector<int32_t>& ks_of, int32_t* pad) {
    int32_t best = -1;
    for (int32_t p = 0; p <= (a > 0 && both + b > 0 ? slack : 0); ++p) {
        int32_t n = 0;
        if (a + both > 0) n += ks_of[(size_t)((both > 0 ? a + p + both : a) - 1) / 32] + 1;
        if (both + b > 0) n += ks_of[(size_t)(a + p + both + b - 1) / 32] - ks_of[(size_t)(a + p) / 32] + 1;
        if (best < 0 || n < best) {
            best = n;
            if (pad) *pad = p;
        }
    }
    return best;
}

// Row assignment for two blocks (32 < T <= 64): which templates share a 32-row block, so that with
// the bit region grouped by block the fewest (K-step, block) fragments are live; on a tie the fewest
// words that touch both blocks. Deterministic local search from two fixed starts ([0, 32) | [32, T),
// and the T - 32 templates of the fewest bit words as block 1), the better end taken: sweeps
// over all swaps of two templates across the blocks and all moves of one template to the other block
// (<= 32 per block), each taken as soon as it improves, until a sweep changes nothing. `rows` holds
// per template a bitset over the n bit words (W 64-bit words each). A block touches the words in the union
// of its rows; with the union of each block without each of its templates at hand (`ex`, rebuilt
// when a move is taken) a candidate costs 2 W ORs and popcounts. Returns block 0's template set.
uint64_t assign_rows(int32_t T, const std::vector<uint64_t>& rows, int32_t W, int32_t n, int32_t slack,
                     const std::vector<int32_t>& ks_of) {
    const uint64_t all = T >= 64 ? ~0ull : (1ull << T) - 1;
    const uint64_t* R = rows.data();
    std::vector<uint64_t> ex((size_t)T * W), full((size_t)2 * W), pre((size_t)(T + 1) * W);
    auto rebuild = [&](uint64_t m0) {
        for (int blk = 0; blk < 2; ++blk) {
            std::vector<int32_t> list;
            for (int32_t i = 0; i < T; ++i)
                if ((int)((m0 >> i) & 1) != blk) list.push_back(i);   // block 0 is the set bits of m0
            const size_t k = list.size();
            std::fill(pre.begin(), pre.begin() + W, 0ull);
            for (size_t x = 0; x < k; ++x)
                for (int32_t w = 0; w < W; ++w) pre[(x + 1) * W + w] = pre[x * W + w] | R[(size_t)list[x] * W + w];
            for (int32_t w = 0; w < W; ++w) full[(size_t)blk * W + w] = pre[k * W + w];
            std::vector<uint64_t> suf((size_t)W, 0ull);
            for (size_t x = k; x-- > 0;) {
                for (int32_t w = 0; w < W; ++w) {
                    ex[(size_t)list[x] * W + w] = pre[x * W + w] | suf[(size_t)w];
                    suf[(size_t)w] |= R[(size_t)list[x] * W + w];
                }
            }
        }
    };
    // cost of block 0 touching x0 | y0 and block 1 touching x1 | y1 (y may be null)
    auto cost = [&](const uint64_t* x0, const uint64_t* y0, const uint64_t* x1, const uint64_t* y1) {
        int32_t p0 = 0, p1 = 0;
        for (int32_t w = 0; w < W; ++w) {
            p0 += __builtin_popcountll(x0[w] | (y0 ? y0[w] : 0ull));
            p1 += __builtin_popcountll(x1[w] | (y1 ? y1[w] : 0ull));
        }
        const int32_t both = p0 + p1 - n;
        return std::make_pair(live_fragments(n - p1, both, n - p0, slack, ks_of, nullptr), both);
    };
    auto search = [&](uint64_t m0) {
        rebuild(m0);
        auto cur = cost(&full[0], nullptr, &full[(size_t)W], nullptr);
        for (int sweep = 0; sweep < 64; ++sweep) {
            bool improved = false;
            auto take = [&](const std::pair<int32_t, int32_t>& c, uint64_t cand) {
                if (!(c < cur)) return;
                cur = c;
                m0 = cand;
                improved = true;
                rebuild(m0);
            };
            for (int32_t i = 0; i < T; ++i) {
                for (int32_t j = i + 1; j < T; ++j) {
                    if (!(((m0 >> i) ^ (m0 >> j)) & 1)) continue;
                    const int32_t i0 = ((m0 >> i) & 1) ? i : j, i1 = i0 == i ? j : i;   // i0 leaves block 0, i1 block 1
                    take(cost(&ex[(size_t)i0 * W], R + (size_t)i1 * W, &ex[(size_t)i1 * W], R + (size_t)i0 * W),
                         m0 ^ (1ull << i) ^ (1ull << j));
                }
                const bool in0 = (m0 >> i) & 1;
                const int n0 = __builtin_popcountll(m0);
                if (in0 ? T - n0 >= 32 : n0 >= 32) continue;   // the other block is full
                if (in0)
                    take(cost(&ex[(size_t)i * W], nullptr, &full[(size_t)W], R + (size_t)i * W), m0 ^ (1ull << i));
                else
                    take(cost(&full[0], R + (size_t)i * W, &ex[(size_t)i * W], nullptr), m0 ^ (1ull << i));
            }
            if (!improved) break;
        }
        return std::make_pair(cur, m0);
    };
    // second start: the T - 32 templates of the fewest bit words in block 1 (index breaks ties)
    std::vector<std::pair<int32_t, int32_t>> weight;
    for (int32_t i = 0; i < T; ++i) {
        int32_t c = 0;
        for (int32_t w = 0; w < W; ++w) c += __builtin_popcountll(R[(size_t)i * W + w]);
        weight.push_back({c, i});
    }
    std::sort(weight.begin(), weight.end());
    uint64_t light = 0;
    for (int32_t k = 0; k < T - 32; ++k) light |= 1ull << weight[(size_t)k].second;
    const auto r0 = search(0xFFFFFFFFull), r1 = search(all & ~light);
    return r1.first < r0.first ? r1.second : r0.second;
}

// Row map and word grouping of a two-block stage. The templates of block 0 (assign_rows) take device
// rows 0.., the others rows 32.., ascending; the bit words are re-placed as the stable partition
// [block 0 only | both | block 1 only] along kstep_dwords, their relative order inside a group as
// place_words left it. Count fields, n_bits and bit_dwords do not change.
void group_bits(const dice_templates* t, const std::vector<uint64_t>& col, CompactLayout& L, MfmaTables& m) {
    const int32_t T = t->n_templates, V = t->n_vocab;
    std::vector<int32_t> ks_of;
    const std::vector<int32_t> seq = kstep_dwords(L.bit_dwords, m.ksteps, ks_of);
    std::vector<int32_t> word((size_t)L.n_bits, -1);   // bit words in their present order
    for (int32_t v = 0; v < V; ++v)
        if (L.dest[(size_t)v] >= 0) word[(size_t)L.dest[(size_t)v]] = v;
    const int32_t W = (L.n_bits + 63) / 64;
    std::vector<uint64_t> rows((size_t)T * W, 0ull);   // per template: the bit words it holds
    for (int32_t k = 0; k < L.n_bits; ++k)
        for (uint64_t c = col[(size_t)word[(size_t)k]]; c; c &= c - 1)
            rows[(size_t)__builtin_ctzll(c) * W + k / 64] |= 1ull << (k % 64);
    const int32_t slack = 32 * L.bit_dwords - L.n_bits;
    const uint64_t all = T >= 64 ? ~0ull : (1ull << T) - 1;
    const uint64_t m0 = assign_rows(T, rows, W, L.n_bits, slack, ks_of), m1 = all & ~m0;
    m.rows.assign(64, -1);
    for (int32_t i = 0, r0 = 0, r1 = 32; i < T; ++i) m.rows[(size_t)(((m0 >> i) & 1) ? r0++ : r1++)] = i;
    std::vector<int32_t> group[3];
    for (int32_t v : word) {
        const bool in0 = (col[(size_t)v] & m0) != 0, in1 = (col[(size_t)v] & m1) != 0;
        group[in0 && in1 ? 1 : in0 ? 0 : 2].push_back(v);
    }
    int32_t pad = 0;
    live_fragments((int32_t)group[0].size(), (int32_t)group[1].size(), (int32_t)group[2].size(), slack, ks_of, &pad);
    int32_t lp = 0;
    for (int g = 0; g < 3; ++g) {
        for (int32_t v : group[g]) {
            L.dest[(size_t)v] = 32 * seq[(size_t)lp / 32] + lp % 32;
            ++lp;
        }
        if (g == 0) lp += pad;
    }
}

// Tile slot of every layout quad.
std::vector<int32_t> slots_of(const std::vector<int32_t>& qperm) {
    std::vector<int32_t> slot_of(qperm.size(), 0);
    for (size_t s = 0; s < qperm.size(); ++s) slot_of[(size_t)qperm[s]] = (int32_t)s;
    return slot_of;
}

// Fragment table and file-side map of a stage shaped by plan_mfma, for the slot order `qperm`.
void build_mfma_tables(const dice_templates* t, const CompactLayout& L, const std::vector<Entry>& entries,
                       const std::vector<int32_t>& qperm, MfmaTables& m) {
    const int32_t T = t->n_templates, qb = (L.bit_dwords + 3) / 4, np = m.ksteps / 4;
    const std::vector<int32_t> slot_of = slots_of(qperm);
    m.slots.assign((size_t)2 * np, -1);
    for (int32_t q = 0; q < qb; ++q) m.slots[(size_t)q] = slot_of[(size_t)q];
    std::vector<uint32_t> mask((size_t)T * std::max(1, L.bit_dwords), 0u);
    for (const Entry& e : entries)
        if (!e.sum) mask[(size_t)e.tpl * L.bit_dwords + e.dword] = e.mask;
    m.frag.assign((size_t)m.ksteps * m.ntiles * 64 * 4, 0u);
    m.map.assign((size_t)m.ksteps * 64, -1);
    std::vector<char> used((size_t)32 * std::max(1, L.bit_dwords), 0);   // bit positions that hold a word
    for (int32_t p : L.dest)
        if (p >= 0) used[(size_t)p] = 1;
    for (int32_t s = 0; s < m.ksteps; ++s) {
        for (int32_t h = 0; h < 2; ++h) {
            const int32_t q = 2 * (s / 4) + h, dw = 4 * q + s % 4;
            if (q >= qb || dw >= L.bit_dwords) continue;
            const int32_t tile_dword = 4 * m.slots[(size_t)q] + s % 4;
            for (int32_t e = 0; e < 32; ++e) {   // element e = 8 k + i: nibble i of fragment dword k, bit 4 i + k
                const int32_t bit = 4 * (e % 8) + e / 8;
                if (used[(size_t)(32 * dw + bit)]) m.map[(size_t)s * 64 + 32 * h + e] = 32 * tile_dword + bit;
            }
            for (int32_t tp = 0; tp < T; ++tp) {
                const uint32_t v = mask[(size_t)tp * L.bit_dwords + dw];
                uint32_t* f = &m.frag[(((size_t)s * m.ntiles + tp / 32) * 64 + 32 * h + tp % 32) * 4];
                f[0] = (v << 2) & 0x44444444u;   // the values paired with widen_a's: 2.0, 1.0, 0.5, 0.5
                f[1] = v & 0x22222222u;
                f[2] = (v >> 2) & 0x11111111u;
                f[3] = (v >> 3) & 0x11111111u;
            }
        }
    }
    // the device table: rows gathered through rows[]; a fragment is live iff it has a non-zero element
    m.dfrag.assign(m.frag.size(), 0u);
    m.live.assign((size_t)m.ksteps * m.ntiles, 0);
    m.n_live = 0;
    for (int32_t s = 0; s < m.ksteps; ++s)
        for (int32_t j = 0; j < m.ntiles; ++j) {
            uint32_t any = 0;
            for (int32_t lane = 0; lane < 64; ++lane) {
                const int32_t tp = m.rows[(size_t)(32 * j + lane % 32)];
                if (tp < 0) continue;
                const uint32_t* src = &m.frag[(((size_t)s * m.ntiles + tp / 32) * 64 + 32 * (lane / 32) + tp % 32) * 4];
                uint32_t* dst = &m.dfrag[(((size_t)s * m.ntiles + j) * 64 + lane) * 4];
                for (int k = 0; k < 4; ++k) any |= dst[k] = src[k];
            }
            m.live[(size_t)s * m.ntiles + j] = any != 0;
            m.n_live += any != 0;
        }
}

// Repack pieces for dice_pack_compact, per tile dword in slot order (`qperm` applied).
std::vector<std::vector<PackPiece>> build_pack_lists(const CompactLayout& L, const std::vector<int32_t>& qperm, int32_t V) {
    const std::vector<int32_t> slot_of = slots_of(qperm);
    auto tile_dword = [&](int32_t d) { return slot_of[(size_t)(d >> 2)] * 4 + (d & 3); };
    struct Key {
        int32_t dst, src, op;
        bool operator<(const Key& o) const {
            return dst != o.dst ? dst < o.dst : src != o.src ? src < o.src : op < o.op;
        }
    };
    std::vector<std::pair<Key, uint32_t>> ps;
    for (int32_t v = 0; v < V; ++v) {
        const int32_t p0 = L.dest[(size_t)v];
        if (p0 == -1) continue;
        Key k;
        k.src = v >> 5;
        if (p0 >= 0) {
            k.dst = tile_dword(p0 >> 5);
            k.op = (p0 & 31) - (v & 31);
        } else {
            const int32_t f = -2 - p0;
            k.dst = tile_dword(L.bit_dwords + f / 4);
            k.op = 64 + 8 * (f % 4);
        }
        ps.push_back({k, 1u << (v & 31)});
    }
    std::stable_sort(ps.begin(), ps.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<std::vector<PackPiece>> lists((size_t)L.quads * 4);
    for (size_t i = 0; i < ps.size(); ++i) {
        const Key& k = ps[i].first;
        std::vector<PackPiece>& l = lists[(size_t)k.dst];
        if (i && !(ps[i - 1].first < k))   // same (dst, src, op): one piece
            l.back().mask |= ps[i].second;
        else
            l.push_back(PackPiece{k.src, ps[i].second, k.op});
    }
    return lists;
}

// ---------------------------------------------------------------------------------------
// Emit: preludes and kernel templates
// ---------------------------------------------------------------------------------------

const char* kPrelude = R"HIP(
typedef unsigned int u32;
typedef int i32;
typedef unsigned long long u64;
typedef long long i64;

#ifdef __HIP_DEVICE_COMPILE__
// v_mul_u32_u24: full-rate 24x24 multiply (low 32 bits); v_sad_u32: |a - b| + c in one op.
__device__ __forceinline__ u32 mul24(u32 a, u32 b) { u32 r; asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ u32 absdiff(u32 a, u32 b) { u32 r; asm("v_sad_u32 %0, %1, %2, 0" : "=v"(r) : "s"(a), "v"(b)); return r; }
__device__ __forceinline__ u32 subsat(u32 a, u32 b) { return __builtin_elementwise_sub_sat(a, b); }   // v_sub_u32 clamp
#else
__device__ __forceinline__ u32 subsat(u32 a, u32 b) { return a > b ? a - b : 0u; }
__device__ __forceinline__ u32 mul24(u32 a, u32 b) { return (a & 0xffffffu) * (b & 0xffffffu); }
__device__ __forceinline__ u32 absdiff(u32 a, u32 b) { return a > b ? a - b : b - a; }
#endif
// acc += popcount(x & MASK): v_and_b32 (literal) + v_bcnt_u32_b32 accumulate. Written as asm
// (ACC_ASM) because the compiler otherwise rebalances the chains into v_bcnt(x, 0) + v_add3.
#if defined(__HIP_DEVICE_COMPILE__) && ACC_ASM
#define ACC_ASM_ONLY(...) __VA_ARGS__
#define ACC_C_ONLY(...)
#else
#define ACC_ASM_ONLY(...)
#define ACC_C_ONLY(...) __VA_ARGS__
#endif
#if defined(__HIP_DEVICE_COMPILE__) && ACC_ASM
#define ACCM(acc, x, MASK) { u32 t_; asm("v_and_b32 %1, " #MASK ", %2\n\tv_bcnt_u32_b32 %0, %1, %0" : "+v"(acc), "=&v"(t_) : "v"(x)); }
#define ACCF1(acc, x) asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x))
#else
#define ACCM(acc, x, MASK) acc = __builtin_popcount((x) & (MASK)) + acc
#define ACCF1(acc, x) acc = __builtin_popcount(x) + acc
#endif
// File-tile quad load; FILE_NT streams it with the non-temporal cache policy (each quad is
// read exactly once per launch).
#if FILE_NT && defined(__HIP_DEVICE_COMPILE__)
typedef u32 u32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ldq(const uint4* p) {
    const u32x4v v = __builtin_nontemporal_load((const u32x4v*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
#else
__device__ __forceinline__ uint4 ldq(const uint4* p) { return *p; }
#endif
#if OUT_NT && defined(__HIP_DEVICE_COMPILE__)
#define MSTORE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define MSTORE(p, v) (*(p) = (v))
#endif
// Denominator (content_helper.rb:130-132,337-347); lengths are non-negative (len_F < 2^31).
__device__ __forceinline__ i32 dn(i32 base, i32 slack, i32 tlen, u32 wf, i32 lf) {
    const u32 d = absdiff((u32)tlen, (u32)lf);
    const u32 adj = slack <= 0 ? d : subsat(d, (u32)slack);   // max(d - slack, 0)
    return base + (i32)wf + (i32)(adj >> 2);
}
__device__ __forceinline__ double sc(u32 o, i32 d) { return ((double)o * 200.0) / (double)d; }
// A fast-path denominator (< 2^21) may carry a template index in bits 24-31 (match kernels): only
// bits 0-23 count there. The IEEE-double path takes whole 32-bit denominators.
template <bool FAST>
__device__ __forceinline__ bool ge(u32 oa, i32 da, u32 ob, i32 db) {
    if (FAST) {
#if NARROW_MUL
        // ov < 2^11 and den < 2^21: both products < 2^32, full-rate 24-bit multiplies are exact
        // (v_mul_u32_u24 reads bits 0-23 of either operand)
        return mul24(oa, (u32)db) >= mul24(ob, (u32)da);
#else
        return (u64)oa * (u64)((u32)db & 0xFFFFFFu) >= (u64)ob * (u64)((u32)da & 0xFFFFFFu);
#endif
    }
    return sc(oa, da) >= sc(ob, db);
}
)HIP";

// Compact tile only: masked four-byte sum of a count dword. The device program (acc_block) does it
// in one v_dot4_u32_u8 against a 0/1-per-byte selector; the plain-C form serves the host tests.
const char* kCompactPrelude = R"HIP(
#ifndef __HIP_DEVICE_COMPILE__
__device__ __forceinline__ u32 bytesum(u32 x) { return (x & 0xffu) + ((x >> 8) & 0xffu) + ((x >> 16) & 0xffu) + (x >> 24); }
#else
__device__ __forceinline__ u32 bytesum(u32 x) { u32 r; asm("v_sad_u8 %0, %1, 0, 0" : "=v"(r) : "v"(x)); return r; }
#endif
#define ACCS(acc, x, MASK) acc = bytesum((x) & (MASK)) + acc
#define ACCSF1(acc, x) acc = bytesum(x) + acc
)HIP";

// MATCH_FILE is the per-file body of both match kernels, from the scalar loads to the three result
// stores; PROLOGUE names the accumulate stage (FILE_PROLOGUE or FILE_PROLOGUE_MFMA). CC_ABOVE and
// CC_BELOW form the cc flag: above the stage in the VALU kernel (MATCH_CC), while the matrix-core
// kernel only requests the byte there, pins the scalar loads, and forms the flag below its stage
// (MFMA_SCALARS_REQUESTED, MFMA_SCALARS_USED).
const char* kMatchKernel = R"HIP(
// Running best: bo = its overlap, bd = its denominator, bi = its template index. On the fast path
// (denominators < 2^21) the index rides in bd's top byte, where the denominator's last add puts it
// for free and the 24-bit multiplies of the compare do not look: one select moves index and
// denominator together, "none yet" is bd = 0xFF000001 with bo = 0 (any candidate is >= 0 / 1), and
// bi comes out of bd behind the last template. The IEEE-double path, whose denominators take all
// 32 bits, keeps bi beside them. AT(p) is the lane's element of a per-file array, IN_RANGE whether
// the lane has a file: each kernel defines both.
#define MATCH_CC const bool cc = *AT(ccp) != 0;
#define MATCH_FILE(PROLOGUE, CC_ABOVE, CC_BELOW) \
    u32 wf = *AT(wfp); \
    i32 lf = *AT(lenp); \
    CC_ABOVE \
    PROLOGUE \
    CC_BELOW \
    const bool fast = CORPUS_FAST && wf < (1u << 20) && lf >= 0 && lf < (1 << 21); \
    u32 bo = 0; i32 bd = (i32)0xFF000001u; i32 bi = -1; \
    if (__all(fast)) { \
        MATCH_BODY(true) \
        bi = ((u32)bd >> 24) == 0xFFu ? -1 : (i32)((u32)bd >> 24); \
        bd &= 0xFFFFFF; \
    } else { \
        bd = 1; \
        MATCH_BODY(false) \
    } \
    if (IN_RANGE) { \
        const double s = bi >= 0 ? sc(bo, bd) : 0.0; \
        MSTORE(AT(best_out), (bi >= 0 && s >= thr) ? bi : -1); \
        MSTORE(AT(ov_out), bo); \
        MSTORE(AT(score_out), s); \
    }
#define AT(p) ((p) + file)
#define IN_RANGE (file < n)
extern "C" __global__ __launch_bounds__(64 * WPB) void dice_prog_match(
    const uint4* __restrict__ files, i64 n, const u32* __restrict__ wfp, const i32* __restrict__ lenp,
    const unsigned char* __restrict__ ccp, double thr, i32* __restrict__ best_out,
    u32* __restrict__ ov_out, double* __restrict__ score_out) {
    const int lane = threadIdx.x & 63;
    const i64 tile = (i64)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (tile * 64 >= n) return;
    const i64 file = tile * 64 + lane;
    const uint4* fp = files + tile * (i64)(WQ * 64) + lane;
#if WAVE_TIMING
    const u64 t0_ = __builtin_amdgcn_s_memrealtime();
#endif
    MATCH_FILE(FILE_PROLOGUE, MATCH_CC, )
#if WAVE_TIMING
    // diagnostics (DICE_PROG_DIAG=timing, results wrong): per wave its start and end real-time (100 MHz)
    // clock and the raw HW_ID / XCC_ID registers, in the tile's first output slots
    const u64 t1_ = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        score_out[tile * 64] = (double)t0_;
        score_out[tile * 64 + 1] = (double)t1_;
        ov_out[tile * 64] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        ov_out[tile * 64 + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
#endif
}
#undef AT
#undef IN_RANGE
)HIP";

// Matrix kernel template: KM is the compile-time top-k slot count (4 or 16). MROWS 1 is the matrix
// kernel (dice_prog_matrix*: every template's overlap and score stored, then the ranking); MROWS 0 is
// the same text without the row pointers, their arguments and the row stores (dice_prog_topk*:
// the ranking alone, dice.rb:34-41 read for its first k entries as detect.rb:96-106 does).
const char* kMatrixKernel = R"HIP(
#if MROWS
#define MROW_ARGS u32* __restrict__ ov_out, double* __restrict__ score_out,
#define MROW_STORE(T) if (valid) { if (orow) MSTORE(orow + (i64)(T) * n, a); if (srow) MSTORE(srow + (i64)(T) * n, sc(a, d)); }
#else
#define MROW_ARGS
#define MROW_STORE(T)
#endif
extern "C" __global__ __launch_bounds__(64 * WPB) void KNAME(
    const uint4* __restrict__ files, i64 n, const u32* __restrict__ wfp, const i32* __restrict__ lenp,
    const unsigned char* __restrict__ ccp, i32 k, MROW_ARGS
    i32* __restrict__ topk_idx, double* __restrict__ topk_score) {
    const int lane = threadIdx.x & 63;
    const i64 tile = (i64)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (tile * 64 >= n) return;
    const i64 file = tile * 64 + lane;
    const bool valid = file < n;
    const uint4* fp = files + tile * (i64)(WQ * 64) + lane;
    const u32 wf = wfp[file];
    const i32 lf = lenp[file];
    const bool cc = ccp[file] != 0;
    FILE_PROLOGUE
    const bool fast = CORPUS_FAST && wf < (1u << 20) && lf >= 0 && lf < (1 << 21);
    i32 ti[KM]; u32 to[KM]; i32 td[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) { ti[j] = -1; to[j] = 0; td[j] = 1; }
#if MROWS
    // template-major [NT][n] outputs: for a fixed template the 64 lanes store contiguously
    u32* orow = ov_out ? ov_out + file : nullptr;
    double* srow = score_out ? score_out + file : nullptr;
#endif
    if (__all(fast)) {
        MATRIX_BODY(true)
    } else {
        MATRIX_BODY(false)
    }
    if (valid && topk_idx) {
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j < k) {
                MSTORE(topk_idx + (i64)j * n + file, ti[j]);
                MSTORE(topk_score + (i64)j * n + file, ti[j] >= 0 ? sc(to[j], td[j]) : -1.0);
            }
        }
    }
}
#undef MROW_ARGS
#undef MROW_STORE
)HIP";

// Per-template matrix epilogue: store the row entry (MROW_STORE, empty in the top-k kernels), then
// rank-and-shift insertion into the KM sorted slots (p = slots that strictly outrank the
// candidate; a later template goes before equal-scored earlier ones, dice.rb:39). Branch-free
// selects only.
const char* kMatrixOffer = R"HIP(
#define MOFFER(T, CCF)                                                                  \
    {                                                                                   \
        MROW_STORE(T)                                                                   \
        if (!((CCF) && cc)) {                                                           \
            int p = 0;                                                                  \
            _Pragma("unroll") for (int j = 0; j < KM; ++j)                              \
                p += (ti[j] >= 0 && !ge<FASTV>(a, d, to[j], td[j])) ? 1 : 0;           \
            _Pragma("unroll") for (int j = KM - 1; j > 0; --j) {                        \
                const bool mv = j > p;                                                  \
                ti[j] = mv ? ti[j - 1] : ti[j];                                         \
                to[j] = mv ? to[j - 1] : to[j];                                         \
                td[j] = mv ? td[j - 1] : td[j];                                         \
            }                                                                           \
            _Pragma("unroll") for (int j = 0; j < KM; ++j) {                            \
                const bool put = j == p;                                                \
                ti[j] = put ? (T) : ti[j];                                              \
                to[j] = put ? a : to[j];                                                \
                td[j] = put ? d : td[j];                                                \
            }                                                                           \
        }                                                                               \
    }
)HIP";

// Matrix-core accumulate stage (device compile only). The bit region of the
// compact tile against the templates' bit masks is a binary matrix product, files x bits times
// bits x templates, so v_mfma_scale_f32_32x32x64_f8f6f4 on e2m1 operands computes a 32-template x
// 32-file block of overlaps per instruction, exactly (every shared bit is 0.5 x 2.0, 1.0 x 1.0 or
// 2.0 x 0.5 at block scale 2^0; counts < 2^24). Templates are the A operand, pre-widened on the
// host (dice_mfma_frag, staged in LDS once per workgroup); files are the B operand: lane (r, h)
// loads whole quads of file 32 m + r -- lane half h takes every other bit quad, a quad's four
// dwords serve four K-steps -- and widens a dword with 5 VALU (widen_a). Accumulator register g of
// lane (c, h) is device row 32 j + (g & 3) + 8 (g >> 2) + 4 h of file 32 m + c, so one
// v_permlane32_swap of the m = 0 and m = 1 registers leaves lane l with two rows' overlaps
// of file l: no LDS transpose. Which template a row holds is the plan's choice (MfmaTables::rows):
// with the bit region grouped by block, a (K-step, block) fragment that is all zero is neither read
// from LDS nor multiplied, and a K-step that is live in no block is not widened. A workgroup of MWK = 12 waves walks a contiguous share of the tiles,
// wave w taking every MWK-th; the next tile's quads are requested as this tile's K-steps retire
// them. Match mode only: the matrix kernels, bound by their 600 B per file of stores, measured
// 17% slower with the stage and keep the VALU program; so do the top-k
// kernels, which store nothing per template but are bound by the slot offers (3% slower, B.6).
const char* kMfmaPrelude = R"HIP(
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ v8i widen_a(u32 v) {
    v8i r;
    r[0] = (int)(v & 0x11111111u);
    r[1] = (int)(v & 0x22222222u);
    r[2] = (int)(v & 0x44444444u);
    r[3] = (int)((v >> 1) & 0x44444444u);
    r[4] = r[5] = r[6] = r[7] = 0;
    return r;
}
__device__ __forceinline__ v8i frag8(uint4 v) {
    v8i r;
    r[0] = (int)v.x; r[1] = (int)v.y; r[2] = (int)v.z; r[3] = (int)v.w;
    r[4] = r[5] = r[6] = r[7] = 0;
    return r;
}
// FP4 x FP4 (cbsz = blgp = 4), block scales 2^0 (E8M0 0x7F in every byte). The scales must be
// VGPRs: given a constant, the runtime compiler folds it into an SGPR operand, which the
// instruction does not take (every product then came out as +inf), so ms_ is made opaque (MFMA_HEAD).
// Observed with hiprtc of ROCm 7.2 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0); the same release's
// offline compiler uses a VGPR. Like ll_ in MFMA_TILE, which keeps the fragment reads inside the tile
// loop, it guards against one compiler's folding and hoisting: tests/test_gpu_prog_mfma.py fails on
// every file with a bit set if either stops working.
#define MFMA44(a, b, c) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, ms_, 0, ms_)
// acc[TA] = overlaps of template TA, acc[TB] = of template TB (rows g and g + 4 of the block),
// lane = file: lanes 32-63 of the m = 0 register swap with lanes 0-31 of the m = 1 register. The
// fold writes the accumulators (a template is folded at most once; one of a block without a live
// fragment keeps its 0) and the count entries behind it add to them.
#define MFMA_FOLD2(C0, C1, G, TA, TB) { typedef u32 u32x2_ __attribute__((ext_vector_type(2))); \
    const u32x2_ r_ = __builtin_amdgcn_permlane32_swap((u32)C0[G], (u32)C1[G], false, false); \
    acc[TA] = r_[0]; acc[TB] = r_[1]; }
#define MFMA_FOLD1(C0, C1, G, TA) { typedef u32 u32x2_ __attribute__((ext_vector_type(2))); \
    const u32x2_ r_ = __builtin_amdgcn_permlane32_swap((u32)C0[G], (u32)C1[G], false, false); \
    acc[TA] = r_[0]; }
#define MFMA_FOLD1B(C0, C1, G, TB) { typedef u32 u32x2_ __attribute__((ext_vector_type(2))); \
    const u32x2_ r_ = __builtin_amdgcn_permlane32_swap((u32)C0[G], (u32)C1[G], false, false); \
    acc[TB] = r_[1]; }
// The compiler sinks a load to its first use when nothing holds it: the scheduling barriers keep
// the tile's loads where the text has them, and the scalars pass through an empty asm below the
// stage, so that their first use (cc != 0 is a compare the compiler would otherwise do at once,
// behind a wait that drains the whole load queue) stays below it.
#define MFMA_PIN __builtin_amdgcn_sched_barrier(0);
#define MFMA_SCALARS_REQUESTED u32 ccr_ = *AT(ccp); MFMA_PIN
#define MFMA_SCALARS_USED asm volatile("" : "+v"(wf), "+v"(lf), "+v"(ccr_)); const bool cc = ccr_ != 0;
// Addresses: a tile's base is wave-uniform and lives on the scalar unit; a lane adds a 32-bit byte
// offset that does not change from tile to tile (its file's place in a quad, a count quad or a
// per-file array), so every load and store of the loop is scalar base + vector offset + immediate.
// The compiler selects that form only where it sees the offset widened next to the access: left
// alone it widens the offsets once above the loop, or carries whole per-lane pointers around it,
// and pays 64-bit vector adds per tile. So each offset passes through an empty asm, in place, in
// the block that uses it (MFMA_QPIN per tile, AT per access): no instruction, one register each.
#define MFMA_AT(base, off) ((const uint4*)((const char*)(base) + (off)))
#define MFMA_ELEM(p, off) ({ asm volatile("" : "+v"(off)); (decltype(p))((char*)((p) + tile * 64) + (off)); })
// Workgroup head: the workgroup's share of the tiles and the wave's first tile, whose quads are
// requested before the template fragments go into LDS and fly during the fill (a wave without a
// tile asks for tile 0, which every launch has, helps with the fill and leaves)
#define MFMA_HEAD \
    __shared__ uint4 tfrag[MFMA_FRAGS * 64]; \
    const u32 lane = threadIdx.x & 63; \
    const i64 nt_ = (n + 63) >> 6; \
    const i64 t1v_ = nt_ * (i64)(blockIdx.x + 1) / (i64)gridDim.x;   /* 64-bit division: vector registers */ \
    const i64 t1 = (i64)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(t1v_ >> 32)) << 32) | \
                         (u32)__builtin_amdgcn_readfirstlane((int)t1v_)); \
    i64 tile = nt_ * (i64)blockIdx.x / (i64)gridDim.x + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); \
    u32 l1_ = lane, l4_ = lane * 4u, l8_ = lane * 8u, l16_ = lane * 16u, ll_ = lane; \
    MFMA_QDECL \
    { const uint4* nb_ = files + (tile < t1 ? tile : 0) * (i64)(WQ * 64); MFMA_PIN MFMA_QLOAD MFMA_PIN } \
    for (int i = threadIdx.x; i < MFMA_FRAGS * 64; i += 64 * MWK) tfrag[i] = ((const uint4*)dice_mfma_frag)[i]; \
    __syncthreads(); \
    if (tile >= t1) return; \
    int ms_ = 0x7F7F7F7F; asm volatile("" : "+v"(ms_));
// Per tile: the quads of the wave's next tile (MFMA_NEXT). After its last tile a wave has none:
// the requests, which keep their place so that the loop has one shape and one count of loads in
// flight, then go to tile 0, which every launch has and every such wave shares.
#define MFMA_TILE \
    const uint4* fb_ = files + tile * (i64)(WQ * 64); \
    const uint4* nb_ = files + (rem_ > MWK ? tile + MWK : 0) * (i64)(WQ * 64); \
    const u32 left_ = tile + 1 != nt_ ? 64u : (u32)(n - tile * 64); \
    MFMA_QPIN asm volatile("" : "+v"(l16_), "+v"(ll_));   /* ll_ opaque: fragment reads stay in the loop (and out of scratch) */
#define MFMA_NEXT(o) MFMA_AT(nb_, o)
// The lane's element of a per-file array: the tile's part of it (scalar) + the lane offset for the
// element size (l1_, l4_, l8_ of MFMA_HEAD; there is none for other sizes).
#define AT(p) ({ \
    static_assert(sizeof(*(p)) == 1 || sizeof(*(p)) == 4 || sizeof(*(p)) == 8, "AT: no lane offset for this element size"); \
    sizeof(*(p)) == 1 ? MFMA_ELEM(p, l1_) : sizeof(*(p)) == 4 ? MFMA_ELEM(p, l4_) : MFMA_ELEM(p, l8_); })
#define IN_RANGE (l1_ < left_)
)HIP";

const char* kMatchKernelMfma = R"HIP(
extern "C" __global__ __launch_bounds__(64 * MWK) void dice_prog_match_mfma(
    const uint4* __restrict__ files, i64 n, const u32* __restrict__ wfp, const i32* __restrict__ lenp,
    const unsigned char* __restrict__ ccp, double thr, i32* __restrict__ best_out,
    u32* __restrict__ ov_out, double* __restrict__ score_out) {
    MFMA_HEAD
    // rem_: the tiles from this one to the end of the workgroup's share (>= 1 here). The scalar unit
    // has no ordered 64-bit compare, so the loop counts in 32 bits; a share of 2^32 tiles is beyond
    // any memory.
    for (u32 rem_ = (u32)(t1 - tile);; rem_ -= MWK, tile += MWK) {
        MFMA_TILE
        MATCH_FILE(FILE_PROLOGUE_MFMA, MFMA_SCALARS_REQUESTED, MFMA_SCALARS_USED)
        if (rem_ <= MWK) break;
    }
}
)HIP";

// ---------------------------------------------------------------------------------------
// Emit: the text generated per corpus
// ---------------------------------------------------------------------------------------

// Emits `text` as the body of a one-line-per-statement macro.
void emit_macro(std::ostringstream& s, const std::string& head, const std::string& text) {
    s << "#define " << head << " \\\n";
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) s << line << " \\\n";
    s << "\n";
}

bool corpus_in_fast_envelope(const dice_templates* t) {
    // static fast-path envelope (dice_common.h): base >= 1, base < 2^18, len < 2^20,
    // 200*|Lf| < 1024*base  =>  every fast-file denominator is in [1, 2^21), scores < 1024.
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const int64_t base = (int64_t)t->lf_size[i] - (int64_t)t->fields_set_size[i];
        if (!(base >= 1 && base < (1 << 18) && t->length[i] >= 0 && t->length[i] < (1 << 20) &&
              200 * (int64_t)t->lf_size[i] < 1024 * base))
            return false;
    }
    return true;
}

// Header comments, the defines the preludes and kernels read, and the preludes.
void emit_defines(std::ostringstream& s, const dice_templates* t, const Program& p) {
    s << "#define WPB " << kProgramWaves << "\n";
    s << "// dice sparse program: T=" << t->n_templates << " V=" << t->n_vocab << " entries=" << p.prog.size() << "\n";
    if (p.opts.compact)
        s << "// layout=compact threshold=" << p.layout.threshold << " bits=" << p.layout.n_bits
          << " bit_dwords=" << p.layout.bit_dwords << " count_bytes=" << p.layout.n_fields << " burst=" << p.opts.burst << "\n";
    uint32_t max_lf = 0;
    for (int32_t i = 0; i < t->n_templates; ++i) max_lf = std::max(max_lf, t->lf_size[i]);
    // v_and/v_bcnt as asm blocks (ACC_ASM; host tests compile the plain-C form), non-temporal file
    // loads (FILE_NT) and outputs (OUT_NT: written once, never re-read; config 5 -1.9%, 3 reps)
    s << "#define ACC_ASM 1\n";
    s << "#define FILE_NT 1\n";
    s << "#define OUT_NT 1\n";
    s << "#define WQ " << p.wq << "\n#define NT " << t->n_templates << "\n#define CORPUS_FAST "
      << (corpus_in_fast_envelope(t) ? 1 : 0) << "\n#define NARROW_MUL " << (max_lf < (1u << 11) ? 1 : 0) << "\n" << kPrelude;
    if (p.opts.compact) s << kCompactPrelude;
    s << "// QPERM";
    for (int32_t q : p.sched.qperm) s << " " << q;
    s << "\n";
}

// One dword-major accumulation statement (plain C; ACC_C_ONLY of acc_block).
std::string acc_stmt(const Entry& en) {
    std::ostringstream o;
    if (en.mask == 0xFFFFFFFFu)
        o << (en.sum ? "ACCSF1" : "ACCF1") << "(acc[" << en.tpl << "], f[" << en.dword % 4 << "]);\n";
    else
        o << (en.sum ? "ACCS" : "ACCM") << "(acc[" << en.tpl << "], f[" << en.dword % 4 << "], 0x" << std::hex
          << en.mask << std::dec << ");\n";
    return o.str();
}

// A block of dword-major accumulations (entries of one quad) as ONE asm statement: the hazard
// recognizer pads every inline-asm boundary with an s_nop, so per-entry asm would cost an
// s_nop per v_and/v_bcnt pair. ACC_C_ONLY carries the plain-C form (host tests, ACC_ASM=0).
// An entry of a count dword is one v_dot4_u32_u8 (acc += sum of byte x selector byte) against the
// mask's 0/1-per-byte selector, a scalar operand: VOP3P takes no literal on gfx950.
// Hazard, kept here because the compiler's recognizer does not look inside an asm statement: on
// gfx950 a VALU instruction other than a dot that reads or writes the destination of a v_dot4 must
// follow it by at least kDotWait wait states (a dot accumulating on a dot needs none). Inside a block
// an s_nop goes in front of such an instruction where other instructions do not fill the distance;
// with `pad_end` (the block's successor is not known to be dots alone) the block ends far enough
// behind its last dots for whatever follows the statement.
constexpr int kDotWait = 3;
std::string acc_block(const std::vector<Entry>& dm, size_t b, size_t e, bool pad_end) {
    std::vector<int32_t> tpls;
    std::vector<int> fk;
    std::vector<uint32_t> sels;
    for (size_t i = b; i < e; ++i) {
        if (std::find(tpls.begin(), tpls.end(), dm[i].tpl) == tpls.end()) tpls.push_back(dm[i].tpl);
        const int k = dm[i].dword % 4;
        if (std::find(fk.begin(), fk.end(), k) == fk.end()) fk.push_back(k);
        const uint32_t sel = dm[i].mask & 0x01010101u;
        if (dm[i].sum && std::find(sels.begin(), sels.end(), sel) == sels.end()) sels.push_back(sel);
    }
    auto acc_op = [&](int32_t tpl) { return (int)(std::find(tpls.begin(), tpls.end(), tpl) - tpls.begin()); };
    // 4 temporaries: the v_and of up to 4 entries issue back to back, then their v_bcnt, so
    // no v_bcnt waits on the v_and right before it
    constexpr int kTmp = 4;
    const int tmp0 = (int)tpls.size();
    auto f_op = [&](int k) { return tmp0 + kTmp + (int)(std::find(fk.begin(), fk.end(), k) - fk.begin()); };
    auto sel_op = [&](uint32_t mask) {
        return tmp0 + kTmp + (int)fk.size() + (int)(std::find(sels.begin(), sels.end(), mask & 0x01010101u) - sels.begin());
    };
    std::ostringstream a, c;
    a << "ACC_ASM_ONLY(asm(\"";
    bool first = true;
    int pos = 0;                                     // wait states issued so far in this block
    std::vector<int> dot_at(tpls.size(), -kDotWait - 1);   // per accumulator: where its last dot was issued
    auto emit = [&](const std::string& ins) {
        if (!first) a << "\\n\\t";
        a << ins;
        first = false;
    };
    auto wait_for = [&](int gap) {                   // s_nop N stands for N + 1 wait states
        if (gap <= 0) return;
        emit("s_nop " + std::to_string(gap - 1));
        pos += gap;
    };
    for (size_t g = b; g < e; g += kTmp) {
        const size_t ge = std::min(e, g + kTmp);
        for (size_t i = g; i < ge; ++i) {
            const Entry& en = dm[i];
            if (en.mask == 0xFFFFFFFFu || en.sum) continue;
            std::ostringstream ins;
            ins << "v_and_b32 %" << tmp0 + (int)(i - g) << ", 0x" << std::hex << en.mask << std::dec << ", %"
                << f_op(en.dword % 4);
            emit(ins.str());
            ++pos;
        }
        for (size_t i = g; i < ge; ++i) {
            const Entry& en = dm[i];
            std::ostringstream ins;
            if (en.sum)
                dot_at[(size_t)acc_op(en.tpl)] = pos;
            else
                wait_for(dot_at[(size_t)acc_op(en.tpl)] + 1 + kDotWait - pos);
            const int src = en.mask == 0xFFFFFFFFu ? f_op(en.dword % 4) : tmp0 + (int)(i - g);
            if (en.sum)   // count dword: sum of the selected bytes
                ins << "v_dot4_u32_u8 %" << acc_op(en.tpl) << ", %" << f_op(en.dword % 4) << ", %" << sel_op(en.mask) << ", %"
                    << acc_op(en.tpl);
            else
                ins << "v_bcnt_u32_b32 %" << acc_op(en.tpl) << ", %" << src << ", %" << acc_op(en.tpl);
            emit(ins.str());
            ++pos;
        }
        for (size_t i = g; i < ge; ++i) c << acc_stmt(dm[i]);
    }
    if (pad_end) wait_for(*std::max_element(dot_at.begin(), dot_at.end()) + 1 + kDotWait - pos);
    a << "\" : ";
    for (size_t i = 0; i < tpls.size(); ++i) a << "\"+v\"(acc[" << tpls[i] << "]), ";
    for (int k = 0; k < kTmp; ++k) a << "\"=&v\"(t_[" << k << "])" << (k + 1 < kTmp ? ", " : "");
    a << " : ";
    for (size_t i = 0; i < fk.size(); ++i) a << (i ? ", " : "") << "\"v\"(f[" << fk[i] << "])";
    for (uint32_t sel : sels) a << ", \"s\"(0x" << std::hex << sel << std::dec << "u)";
    a << ");)";
    std::string cs = c.str();
    std::replace(cs.begin(), cs.end(), '\n', ' ');
    return "{ u32 t_[4]; " + a.str() + " ACC_C_ONLY(" + cs + ") (void)t_; }\n";
}

// Accumulations of the entries [b0, end) of the quad in tile slot `slot`, in blocks of at most
// kAccBlock entries. A block is padded for the dot hazard (acc_block) unless the next block of the
// quad holds count entries only; what follows the quad's last block is not known here.
std::string acc_quad(const Program& p, size_t b0, size_t end, size_t slot) {
    constexpr size_t kAccBlock = 4;   // entries per asm block (2 and 8 measured slower)
    if (p.opts.diag == ProgramOptions::kNoAcc) return "acc[" + std::to_string(slot) + " % NT] ^= f[0] ^ f[1] ^ f[2] ^ f[3];\n";
    std::string out;
    for (size_t b = b0; b < end; b += kAccBlock) {
        const size_t be = std::min(end, b + kAccBlock);
        bool pad_end = be == end;
        for (size_t i = be; i < std::min(end, be + kAccBlock); ++i) pad_end = pad_end || !p.sched.dm[i].sum;
        out += acc_block(p.sched.dm, b, be, pad_end);
    }
    return out;
}

const char* kAccDecl = "u32 acc[NT];\n_Pragma(\"unroll\") for (int i = 0; i < NT; ++i) acc[i] = ACC_INIT(i);\n";

// FILE_PROLOGUE, the VALU stream: slots in groups of `nb` = 5, double-buffered in register sets
// p0_* / p1_*; group g+1 is requested (nb contiguous 1 KiB wave loads back to back) before group g
// is consumed. With non-temporal loads, bursts of 3 measured ~1.5% ahead of an 8-deep
// ring at 92 instead of 124 VGPRs, 4 another ~3.5%, 5 another 1.8% (6: -0.3%)
std::string valu_prologue(const Program& p) {
    const size_t ns = p.sched.range.size();
    const int nb = std::max(1, std::min<int>(p.opts.burst, (int)ns));
    const size_t ng = (ns + nb - 1) / nb;
    std::ostringstream o;
    auto group_loads = [&](size_t g, int set) {
        for (size_t i = g * nb; i < std::min(ns, (g + 1) * nb); ++i)
            o << "p" << set << "_" << (i - g * nb) << " = ldq(fp + " << i * 64 << "); ";
        o << "\n";
    };
    o << kAccDecl;
    for (int i = 0; i < nb; ++i) o << "uint4 p0_" << i << ", p1_" << i << ";\n";
    group_loads(0, 0);
    for (size_t g = 0; g < ng; ++g) {
        const int cur = (int)(g % 2), nxt = 1 - cur;
        o << "__builtin_amdgcn_sched_barrier(0);\n";
        if (g + 1 < ng) group_loads(g + 1, nxt);
        o << "__builtin_amdgcn_sched_barrier(0);\n";
        for (size_t i = g * nb; i < std::min(ns, (g + 1) * nb); ++i) {
            o << "{ const uint4 v = p" << cur << "_" << (i - g * nb) << "; const u32 f[4] = {v.x, v.y, v.z, v.w};\n";
            o << acc_quad(p, p.sched.range[i].first, p.sched.range[i].second, i);
            o << "}\n";
        }
    }
    return o.str();
}

// FILE_PROLOGUE_MFMA, the matrix-core form of the prologue (kMfmaPrelude): count quads requested
// lane per file, the live K-steps pair by pair of bit quads (one fragment read and two matrix
// instructions per live block) with the next tile's pair requested behind them, the fold into acc[]
// through the row map, then the count entries as in the VALU program. With it the MFMA_QDECL
// and MFMA_QLOAD macros: per-lane byte offsets into a tile (lane half h takes the odd quad of each
// pair; l16_ is the lane's place in a count quad), declarations, loads from the tile at nb_, and
// MFMA_QPIN (kMfmaPrelude).
void emit_mfma_prologue(std::ostringstream& s, const dice_templates* t, const Program& p) {
    const MfmaTables& m = p.mf;
    const std::vector<Entry>& dm = p.sched.dm;
    const int32_t np = m.ksteps / 4, nj = m.ntiles;
    const size_t ns = p.sched.range.size();
    std::ostringstream o;
    o << kAccDecl;
    std::vector<std::pair<size_t, size_t>> crange(ns, {0, 0});   // count entries per slot
    for (size_t i = 0; i < ns; ++i) {
        size_t b = p.sched.range[i].first;
        while (b < p.sched.range[i].second && !dm[b].sum) ++b;
        crange[i] = {b, p.sched.range[i].second};
        if (b < p.sched.range[i].second) o << "const uint4 cq_" << i << " = ldq(MFMA_AT(fb_, l16_) + " << i * 64 << ");\n";
    }
    o << "MFMA_PIN\n";   // the count quads are requested here, above the K-steps
    // DICE_PROG_DIAG=nomfma (results wrong): neither fragment reads nor matrix instructions; the
    // widened file operands and the accumulators are kept alive through empty asm statements
    const bool no_mfma = p.opts.diag == ProgramOptions::kNoMfma;
    std::vector<char> blive((size_t)nj, 0);   // blocks with a live fragment: the others have no accumulators
    for (int32_t ks = 0; ks < m.ksteps; ++ks)
        for (int32_t j = 0; j < nj; ++j) blive[(size_t)j] |= m.live[(size_t)ks * nj + j];
    for (int32_t j = 0; j < nj; ++j) {
        if (!blive[(size_t)j]) continue;
        o << "v16f c" << j << "_0 = {}, c" << j << "_1 = {};\n";
        if (no_mfma) o << "asm volatile(\"\" : \"+v\"(c" << j << "_0), \"+v\"(c" << j << "_1));\n";
    }
    const char* comp = "xyzw";
    for (int32_t u = 0; u < np; ++u) {
        for (int32_t d = 0; d < 4; ++d) {
            const int32_t ks = 4 * u + d;
            bool any = false;
            for (int32_t j = 0; j < nj; ++j) any = any || m.live[(size_t)ks * nj + j];
            if (!any) continue;   // live in no block: not widened
            o << "{ const v8i b0_ = widen_a(q0_" << u << "." << comp[d] << "), b1_ = widen_a(q1_" << u << "."
              << comp[d] << ");\n";
            if (no_mfma)
                o << "asm volatile(\"\" :: \"v\"(b0_[0]), \"v\"(b0_[1]), \"v\"(b0_[2]), \"v\"(b0_[3]), \"v\"(b1_[0]), "
                     "\"v\"(b1_[1]), \"v\"(b1_[2]), \"v\"(b1_[3]));\n";
            for (int32_t j = 0; j < nj && !no_mfma; ++j) {
                if (!m.live[(size_t)ks * nj + j]) continue;
                o << "{ const v8i a_ = frag8(tfrag[" << (ks * nj + j) * 64 << " + ll_]); c" << j << "_0 = MFMA44(a_, b0_, c"
                  << j << "_0); c" << j << "_1 = MFMA44(a_, b1_, c" << j << "_1); }\n";
            }
            o << "}\n";
        }
        // the pair's registers are free: the next tile's pair, held in place
        o << "MFMA_PIN\nq0_" << u << " = ldq(MFMA_NEXT(o_" << u << ")); q1_" << u << " = ldq(MFMA_NEXT(o_" << u
          << ") + 32);\nMFMA_PIN\n";
    }
    // the fold names the templates through the row map: a pad can sit on either side of a pair
    for (int32_t j = 0; j < nj; ++j)
        for (int32_t g = 0; g < 16 && blive[(size_t)j]; ++g) {
            const int32_t ra = 32 * j + (g & 3) + 8 * (g >> 2);
            const int32_t ta = m.rows[(size_t)ra], tb = m.rows[(size_t)ra + 4];
            if (ta < 0 && tb < 0) continue;
            o << (ta >= 0 && tb >= 0 ? "MFMA_FOLD2" : ta >= 0 ? "MFMA_FOLD1" : "MFMA_FOLD1B") << "(c" << j << "_0, c" << j
              << "_1, " << g;
            if (ta >= 0) o << ", " << ta;
            if (tb >= 0) o << ", " << tb;
            o << ")\n";
        }
    for (size_t i = 0; i < ns; ++i) {
        if (crange[i].first == crange[i].second) continue;
        o << "{ const u32 f[4] = {cq_" << i << ".x, cq_" << i << ".y, cq_" << i << ".z, cq_" << i << ".w};\n";
        o << acc_quad(p, crange[i].first, crange[i].second, i);
        o << "}\n";
    }
    std::ostringstream qd, ql;
    for (int32_t u = 0; u < np; ++u) {
        const int32_t s0 = m.slots[(size_t)2 * u], s1 = m.slots[(size_t)2 * u + 1] >= 0 ? m.slots[(size_t)2 * u + 1] : s0;
        qd << "u32 o_" << u << " = (((lane >> 5) ? " << s1 * 64 << "u : " << s0 * 64 << "u) + (lane & 31)) * 16u; uint4 q0_"
           << u << ", q1_" << u << ";\n";
        ql << "q0_" << u << " = ldq(MFMA_NEXT(o_" << u << ")); q1_" << u << " = ldq(MFMA_NEXT(o_" << u << ") + 32);\n";
    }
    std::ostringstream qp;
    qp << "asm volatile(\"\" : ";
    for (int32_t u = 0; u < np; ++u) qp << (u ? ", " : "") << "\"+v\"(o_" << u << ")";
    qp << ");\n";
    emit_macro(s, "MFMA_QPIN", qp.str());
    emit_macro(s, "MFMA_QDECL", qd.str());
    emit_macro(s, "MFMA_QLOAD", ql.str());
    emit_macro(s, "FILE_PROLOGUE_MFMA", o.str());
}

// MATCH_BODY and MATRIX_BODY: per template its denominator, then the offer to the running best
// (match) or to the row and the top-k slots (MOFFER).
void epilogue_bodies(const dice_templates* t, const Program& p, std::string& match_body, std::string& matrix_body) {
    std::ostringstream mb, xb;
    // The fast path's index byte (MATCH_FILE) holds indices up to kMaxIndexedTemplates - 1: 0xFF is "none
    // yet". The literal is formed unsigned, so an index above 127 wraps into a negative i32 whose bits are right.
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const int32_t base = (int32_t)t->lf_size[i] - (int32_t)t->fields_set_size[i];
        std::ostringstream den;
        den << "{ const u32 a = acc[" << i << "]; i32 d; d = dn(" << base << ", " << t->length_slack[i] << ", "
            << t->length[i] << ", wf, lf); ";
        // match, fast path: d carries the template index in its top byte, added with the literal
        // base (MATCH_FILE); the IEEE-double path keeps whole denominators and bi beside them
        mb << "{ const u32 a = acc[" << i << "]; const i32 d = dn(FASTV ? " << (int32_t)((uint32_t)base + ((uint32_t)i << 24)) << " : " << base << ", "
           << t->length_slack[i] << ", " << t->length[i] << ", wf, lf); " << (t->is_cc[i] ? "if (!cc) " : "")
           << "{ if (FASTV) { if (ge<true>(a, d, bo, bd)) { bo = a; bd = d; } } else if (bi < 0 || ge<false>(a, d, bo, bd)) "
              "{ bo = a; bd = d; bi = " << i << "; } } }\n";
        xb << den.str() << "MOFFER(" << i << ", " << (t->is_cc[i] ? 1 : 0) << ") }\n";
    }
    match_body = mb.str();
    if (p.opts.diag == ProgramOptions::kNoEpi)
        match_body = "bd = 1; bo = 0; bi = 0; _Pragma(\"unroll\") for (int i = 0; i < NT; ++i) bo += acc[i];\n";
    matrix_body = xb.str();
}

// The repack kernel of the compact tile, generated beside the program (device compile only: the
// host tests pack their tiles in numpy). One workgroup per 64-file tile stages the tile's rows
// through LDS with coalesced 8-byte loads (row stride odd in dwords, so the 64 lanes of a wave,
// one file each, hit distinct banks; rows too long for 64 KiB are read from global memory
// instead), then each of its four waves builds whole quads -- row dwords at constant LDS
// offsets, masks and shifts as literals -- and stores one uint4 per lane. Quads are dealt to
// the waves by piece count, largest first.
void emit_pack_kernel(std::ostringstream& s, const Program& p, int32_t w64) {
    const CompactLayout& L = p.layout;
    int32_t stride = (2 * w64) | 1;
    if ((size_t)64 * stride * 4 > 64 * 1024) stride = 0;
    s << "#ifdef __HIP_DEVICE_COMPILE__\n#define PACK_STRIDE " << stride << "\n#define PACK_W64 " << w64 << "\n";
    s << R"HIP(extern "C" __global__ __launch_bounds__(256) void dice_pack_compact(
    const u64* __restrict__ rows, i64 n, uint4* __restrict__ tiles) {
    const i64 tile = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const i64 file0 = tile * 64;
    const bool valid = file0 + lane < n;
#if PACK_STRIDE
    __shared__ u32 lrows[64 * PACK_STRIDE];
    {
        const i64 left = n - file0;
        const int nvalid = left < 64 ? (int)left : 64;
        const u64* src = rows + file0 * PACK_W64;
        for (int i = threadIdx.x; i < 64 * PACK_W64; i += 256) {
            const int f = i / PACK_W64, d = i - f * PACK_W64;
            const u64 x = f < nvalid ? src[i] : 0ull;
            lrows[f * PACK_STRIDE + 2 * d] = (u32)x;
            lrows[f * PACK_STRIDE + 2 * d + 1] = (u32)(x >> 32);
        }
        __syncthreads();
    }
    const u32* r = lrows + lane * PACK_STRIDE;
#else
    const u32* r = (const u32*)(rows + (valid ? file0 + lane : file0) * PACK_W64);
#endif
    uint4* out = tiles + tile * (i64)(WQ * 64) + lane;
#define PC(src, m) ((u32)__builtin_popcount(r[src] & (m)))
#define PUT(slot, a, b, c, d) out[(slot) * 64] = valid ? make_uint4(a, b, c, d) : make_uint4(0, 0, 0, 0);
    switch (wave) {
)HIP";
    // quads to waves: largest piece count first, to the wave with the least so far
    std::vector<std::pair<size_t, int32_t>> order;
    for (int32_t q = 0; q < L.quads; ++q) {
        size_t np = 0;
        for (int k = 0; k < 4; ++k) np += p.pack_lists[(size_t)q * 4 + k].size();
        order.push_back({np, q});
    }
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    std::vector<int32_t> of_wave[4];
    size_t load[4] = {0, 0, 0, 0};
    for (const auto& o : order) {
        const int w = (int)(std::min_element(load, load + 4) - load);
        of_wave[w].push_back(o.second);
        load[w] += o.first + 1;
    }
    for (int w = 0; w < 4; ++w) {
        s << "    case " << w << ":\n";
        for (int32_t q : of_wave[w]) {
            s << "        PUT(" << q;
            for (int k = 0; k < 4; ++k) {
                const std::vector<PackPiece>& l = p.pack_lists[(size_t)q * 4 + k];
                s << ",\n            ";
                if (l.empty()) {
                    s << "0u";
                } else if (l[0].op >= 64) {   // count dword: popcounts summed per byte
                    bool first = true;
                    for (int by = 0; by < 4; ++by) {
                        std::ostringstream sum;
                        for (const PackPiece& pc : l) {
                            if (pc.op != 64 + 8 * by) continue;
                            sum << (sum.tellp() > 0 ? " + " : "") << "PC(" << pc.src << ", 0x" << std::hex << pc.mask
                                << std::dec << "u)";
                        }
                        if (sum.tellp() <= 0) continue;
                        s << (first ? "" : " + ") << "((" << sum.str() << ") << " << 8 * by << ")";
                        first = false;
                    }
                } else {
                    for (size_t i = 0; i < l.size(); ++i) {
                        const PackPiece& pc = l[i];
                        s << (i ? " | " : "") << "((r[" << pc.src << "] & 0x" << std::hex << pc.mask << std::dec << "u)";
                        if (pc.op > 0) s << " << " << pc.op;
                        if (pc.op < 0) s << " >> " << -pc.op;
                        s << ")";
                    }
                }
            }
            s << ")\n";
        }
        s << "        break;\n";
    }
    s << "    }\n#undef PC\n#undef PUT\n}\n#endif\n";
}

}  // namespace

Program plan_program(const dice_templates* t, const ProgramOptions& opts) {
    Program p;
    p.opts = opts;
    const int32_t w64 = (t->n_vocab + 63) / 64;
    std::vector<uint64_t> col;   // compact tile: template-membership column per word
    if (opts.compact) {
        col = word_columns(t);
        derive_layout(t, col, p.layout, p.prog);
        p.wq = p.layout.quads;
    } else {
        p.prog = build_entries(t, w64);
        p.wq = (w64 + 1) / 2;
    }
    if (opts.compact) {
        plan_mfma(t, p.layout, p.mf);
        if (p.mf.eligible && p.mf.ntiles == 2) {   // two blocks: rows assigned, the bit region grouped by block
            group_bits(t, col, p.layout, p.mf);
            build_compact_entries(t, col, p.layout, p.prog);
        }
    }
    p.sched = build_schedule(p.prog, p.wq);
    if (opts.compact) {
        if (p.mf.eligible) build_mfma_tables(t, p.layout, p.prog, p.sched.qperm, p.mf);
        cost_mfma(t, p.prog, p.mf);
        p.mfma_forced = opts.match == ProgramOptions::kMfma && p.mf.eligible;
        p.mfma = p.mfma_forced || (opts.match != ProgramOptions::kValu && p.mf.pays);
        p.pack_lists = build_pack_lists(p.layout, p.sched.qperm, t->n_vocab);
    }
    return p;
}

std::string emit_program(const dice_templates* t, const Program& p) {
    std::ostringstream s;
    std::string match_body, matrix_body;
    epilogue_bodies(t, p, match_body, matrix_body);
    emit_defines(s, t, p);
    emit_macro(s, "FILE_PROLOGUE", valu_prologue(p));
    s << "#define WAVE_TIMING " << (p.opts.diag == ProgramOptions::kTiming ? 1 : 0) << "\n";
    emit_macro(s, "MATCH_BODY(FASTV_) { constexpr bool FASTV = FASTV_;", match_body + "}");
    s << "#define ACC_INIT(i) 0u\n" << kMatchKernel;
    s << kMatrixOffer;
    emit_macro(s, "MATRIX_BODY(FASTV_) { constexpr bool FASTV = FASTV_;", matrix_body + "}");
    for (int rows : {1, 0}) {
        for (int km : {4, 16}) {
            s << "#define KM " << km << "\n#define MROWS " << rows << "\n#define KNAME dice_prog_"
              << (rows ? "matrix" : "topk") << km << "\n" << kMatrixKernel << "#undef KM\n#undef MROWS\n#undef KNAME\n";
        }
    }
    if (p.mfma) {
        // the match kernel with the matrix-core accumulate stage, device compile only
        s << "// matrix-core stage: ksteps=" << p.mf.ksteps << " blocks=" << p.mf.ntiles << " live=" << p.mf.n_live
          << " valu_cost=" << p.mf.valu_cost << " stage_cost=" << p.mf.stage_cost << "\n";
        s << "#ifdef __HIP_DEVICE_COMPILE__\n#define MFMA_FRAGS " << p.mf.ksteps * p.mf.ntiles << "\n";
        s << "__device__ const u32 dice_mfma_frag[" << p.mf.dfrag.size() << "] __attribute__((aligned(16))) = {\n" << std::hex;
        for (size_t i = 0; i < p.mf.dfrag.size(); ++i) s << "0x" << p.mf.dfrag[i] << (i % 16 == 15 ? ",\n" : ",");
        s << std::dec << "};\n" << kMfmaPrelude;
        emit_mfma_prologue(s, t, p);
        s << "#define MWK " << kMfmaMatchWaves << "\n" << kMatchKernelMfma << "#undef AT\n#undef IN_RANGE\n#endif\n";
    }
    if (p.opts.compact) emit_pack_kernel(s, p, (t->n_vocab + 63) / 64);
    return s.str();
}

}  // namespace dice
