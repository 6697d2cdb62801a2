// Internal definitions shared by dice.hip and dice_program.cpp (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/licensee_dice.h"
#include "dice_program.h"

namespace dice {

constexpr int32_t kProgramMaxTemplates = 64;   // sparse program kernel for T <= 64

// thread-local last-error text (dice_last_error)
std::string& last_error();

inline int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}

// Diagnostic switches (DICE_*_DIAG) make results wrong by design (phase-skip and timing
// builds). They are honoured only by a library built with -DDICE_DIAG; the
// shipped library ignores them and says so once on stderr, so a stray variable in a production
// environment cannot corrupt Dice#match output.
inline const char* diag_env(const char* name) {
    const char* v = getenv(name);
    if (!v || !*v) return nullptr;
#ifdef DICE_DIAG
    return v;
#else
    static bool warned = false;
    if (!warned) {
        warned = true;
        fprintf(stderr, "liblicensee_dice: %s=%s ignored (diagnostic switches need a -DDICE_DIAG build)\n", name, v);
    }
    return nullptr;
#endif
}

// ---- device plumbing: the one set-device guard, the one HIP check, the one owner of device memory ----

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return ::dice::fail(DICE_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

// Move-only owner of one device allocation of `count` elements (a byte buffer, DevBytes, where the
// element type lives in another file), or a non-owning window into another buffer (view).
// reserve(count) frees without waiting and reserve(count, stream) waits for `stream` first: the second
// form stands where the code always waited for the stream that may still read the buffer; whether the
// others need a wait is unknown -- they lean on hipFree, which waits for the device's work itself.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
    bool owned_ = true;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), owned_(o.owned_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {   // (what this held goes with `o`)
        std::swap(p_, o.p_), std::swap(cap_, o.cap_), std::swap(owned_, o.owned_);
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_ && owned_) (void)hipFree(p_);
        p_ = nullptr, cap_ = 0, owned_ = true;
    }
    // no-op while the capacity suffices; a count of 0 allocates one element
    int reserve(size_t count) {
        if (p_ && cap_ >= count) return DICE_OK;
        reset();
        if (hipMalloc(reinterpret_cast<void**>(&p_), (count ? count : 1) * sizeof(T)) != hipSuccess) {
            p_ = nullptr;
            return fail(DICE_E_NOMEM, "hipMalloc failed");
        }
        cap_ = count;
        return DICE_OK;
    }
    int reserve(size_t count, hipStream_t sync_first) {
        if (p_ && cap_ >= count) return DICE_OK;
        if (hipStreamSynchronize(sync_first) != hipSuccess) return fail(DICE_E_DEVICE, "hipStreamSynchronize failed");
        return reserve(count);
    }
    void view(T* p, size_t count) {
        reset();
        p_ = p, cap_ = count, owned_ = false;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T** arg() { return &p_; }   // a hipModuleLaunchKernel argument: the address of the stored pointer
    DevBuf* operator&() = delete;   // ... which &buf would silently not be
};
using DevBytes = DevBuf<unsigned char>;

}  // namespace dice

struct dice_ctx {
    int device = 0;
    int32_t T = 0, V = 0, w64 = 0, wq = 0, tpad = 0;
    hipStream_t stream = nullptr;
    // Device memory: every d_* field of the context and of the batch is a DevBuf, freed by the
    // struct's destructor (ctx_free and dice_batch_destroy keep no list)
    dice::DevBuf<uint4> d_tq;   // [wq][tpad] template quads (dense kernel)
    dice::DevBuf<int4> d_tc;    // [tpad] TplConst (dense kernel)
    int32_t kind = 0;       // 0 dense, 1 sparse program, 2 LDS-tiled records, 3 postings (T > 64)
    dice::Program prog;     // sparse program (kind 1)
    hipModule_t module = nullptr;
    hipFunction_t prog_match = nullptr;
    hipFunction_t prog_matrix = nullptr;    // top-k <= 4
    hipFunction_t prog_matrix16 = nullptr;  // top-k <= 16
    hipFunction_t prog_topk = nullptr;      // the ranking without the N x T rows, top-k <= 4
    hipFunction_t prog_topk16 = nullptr;    // top-k <= 16
    hipFunction_t prog_match_mfma = nullptr;   // prog_match with the matrix-core accumulate stage (prog.mfma)
    dice::DevBuf<int32_t> d_qperm;          // sparse program tile slot -> vocabulary quad (kind 1)
    // Quads per file of the resident tile: wq (the row's quads) except for the sparse program's
    // compact tile, which the generated dice_pack_compact fills (dice_program.cpp).
    int32_t twq = 0;
    hipFunction_t prog_pack = nullptr;      // compact tile only
    dice_batch* scratch = nullptr;  // reused by the host-buffer calls
    // kind 2 plan (dice_lds.hip): per-(slab, template) entry runs, entries, wave split
    dice::DevBytes d_lrec, d_lep, d_lwt;
    int32_t lds_nslab = 0, lds_npass = 0;
    int64_t lds_entries = 0;
    // kind 3 plan (dice_post.hip): postings rows of the narrow words, dense-prefix masks
    dice::DevBytes d_pdmt;     // [20][kMfmaCols] u64 dense-prefix masks, word-major, zero-padded (MFMA kernel)
    dice::DevBytes d_prow;     // [64*w64][16] u16 postings row per word (short ids / long word ref)
    dice::DevBytes d_povf;     // flat u16 template ids of the long words
    dice::DevBytes d_ptc;      // [T] int4 template constants
    int32_t post_dense = 0, post_tpad = 0, post_tp = 0, post_ld = 0;
    bool post_fast = false;
    int64_t post_rows = 0;
    // kind 3 match mode, bound-pruned (dice_prune.hip): tables in position (length-sorted) order --
    // group bytes, constants, CC masks, template index | record offset, records, slot bounds
    bool prune = false, prune_zero_base = false;
    uint32_t prune_max_lf = 0;       // largest template |Lf| (the long-file test of dice_match's routing)
    int32_t prune_long_route = 4;    // dice_match: postings kernels when >= 1/N of a batch's files are long (0: never)
    uint32_t prune_wf_noclamp = 0;   // |W_F| from which the bound's length term needs no clamp
    dice::DevBytes d_p4q8, d_p4tc, d_p4cc, d_p4off, d_p4rec, d_p4slot;
    int32_t p4_zkeep[2] = {-1, -1}, p4_zpos[2] = {0, 0};
    int32_t n_cu = 256, prune_max_evals = 8, prune_route = 16;
    // sharded calls (dice_shard.cpp): devices this ctx's device has peer access to (bit d), and
    // two page-locked staging buffers for shard uploads from pageable caller memory
    uint64_t peer_mask = 0;
    void* h_stage[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    size_t h_stage_bytes = 0;
    // Exact matcher (dice_exact.hip): host copy of the Lf bitsets; templates sorted by |W_t|
    // {|W_t|, t, record range}, need masks, records of W_t ∩ V
    std::vector<uint64_t> h_lf;
    // small host-buffer calls (n <= kSmallFiles, dice.hip): a batch whose inputs and results are
    // each one device region, mirrored by page-locked host regions -- one H2D and one D2H per call
    dice_batch* small = nullptr;
    void *h_small_in = nullptr, *h_small_out = nullptr;
    dice::DevBytes d_ex_tbl, d_ex_need, d_ex_rec;
    bool exact_ready = false;
    // device wordset scan (dice_words.hip): the vocabulary table -- tagged slots, keys, lengths,
    // word offsets and bytes (for long words' tails)
    dice::DevBytes d_wslots, d_wkeys, d_wlen, d_woff, d_wtxt;
    uint32_t words_bmask = 0, words_id_bits = 0, words_extra = 0;
    bool words_ready = false;
};

namespace dice {
int lds_setup(dice_ctx* c, const dice_templates* t);
int lds_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s);
bool post_feasible(const dice_templates* t);
int post_setup(dice_ctx* c, const dice_templates* t);
// confidence: Dice#confidence outputs (overlap 0 and score 0.0 for a file without a match)
int post_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s, bool confidence = false);
int post_launch_matrix(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s);
// the same ranking into the [n][k] buffers alone: no N x T row is written (dice_batch_topk)
int post_launch_topk(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s);
// the deferred files idx[0 .. *pn) of a pruned match (count on the device; no host read-back)
int post_launch_match_indexed(dice_ctx* c, dice_batch* b, double thr, const int32_t* idx, const uint32_t* pn,
                              hipStream_t s, bool confidence = false);
// the batch's dense-partial buffer ([capacity][tp] u16)
int post_reserve(dice_ctx* c, dice_batch* b);
int prune_setup(dice_ctx* c, const dice_templates* t);
int prune_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s, bool confidence = false);
// the pruned match's device buffers for batch b (called by dice_batch_create)
int prune_reserve(dice_ctx* c, dice_batch* b);
// dice_batch_upload's tail (scalars, repack) for rows already copied to b->d_rows on `s`
int upload_rows_resident(dice_batch* b, const dice_files* f, hipStream_t s);
// the ctx's reusable batch for the host-buffer calls (grown on demand)
int scratch_for(dice_ctx* ctx, int64_t n, dice_batch** out);
// result downloads to host memory or (kind hipMemcpyDefault) another device's memory;
// synchronize `s`
int download_match_to(dice_batch* b, int32_t* best, uint32_t* ov, double* score, hipStream_t s,
                      hipMemcpyKind kind);
int download_matrix_to(dice_batch* b, uint32_t* ov, double* score, int32_t* tki, double* tks, hipStream_t s,
                       hipMemcpyKind kind);
int download_topk_to(dice_batch* b, int32_t* tki, double* tks, hipStream_t s, hipMemcpyKind kind);
// dice_batch_upload's tail: per-file scalars (wf == NULL: already on the device, b->n_long set;
// len == NULL: already on the device), padding, and the tile repack (dice.hip)
int upload_tail(dice_batch* b, int64_t n, const uint32_t* wf, const int32_t* len, const uint8_t* cc, hipStream_t s);
// the tile-layout kernels' repack of b->d_rows (no-op for the postings kernels)
int repack(dice_batch* b, hipStream_t s);
}  // namespace dice

struct dice_batch {
    dice_ctx* ctx = nullptr;
    int64_t capacity = 0, n = 0, n_tiles_cap = 0;
    dice::DevBuf<uint64_t> d_rows;  // staging [capacity][w64]
    dice::DevBuf<uint4> d_tiles;    // [n_tiles][wq][64]
    dice::DevBuf<uint32_t> d_wf;
    dice::DevBuf<int32_t> d_len;
    dice::DevBuf<uint8_t> d_cc;
    dice::DevBuf<int32_t> d_best;
    dice::DevBuf<uint32_t> d_ov;
    dice::DevBuf<double> d_score;
    // matrix results (lazily allocated: [capacity][mat_ld] and [capacity][k] entries)
    int32_t k_used = 0;
    int32_t rank_mode = 0;          // last ranking call: 0 none, 1 dice_batch_matrix, 2 dice_batch_topk
    bool mat_rowmajor = false;      // kind 3 writes [n][ld] / [n][k] directly (no transpose)
    int32_t mat_ld = 0;             // row stride (templates) of the row-major matrix
    dice::DevBuf<uint32_t> d_mov;   // template-major [T][capacity] (coalesced stores)
    dice::DevBuf<double> d_mscore;  // template-major [T][capacity]
    dice::DevBuf<int32_t> d_tki;
    dice::DevBuf<double> d_tks;
    dice::DevBytes d_stage;         // row-major staging for downloads
    dice::DevBytes d_pdense;        // kind 3: dense-prefix partial overlaps [capacity][tp] u16
    dice::DevBytes d_ids;           // dice_batch_upload_ids staging: the id list ...
    dice::DevBuf<int64_t> d_offs;   // ... and its [capacity + 1] offsets
    // pruned match (dice_prune.hip): files deferred to the postings kernels
    dice::DevBuf<int32_t> d_defer;  // [capacity] file indices dice_prune4 deferred
    dice::DevBuf<uint32_t> d_ndefer;   // their count
    dice::DevBuf<uint32_t> d_nscored;  // per wave of the last pruned launch: (file, template) pairs scored exactly
    int64_t prune_waves = 0;        // waves of that launch (entries of d_nscored)
    int32_t last_match = 0;         // last match call: 0 none, 1 every pair scored, 2 bound-pruned
    int64_t n_long = 0;             // files of the upload with |W_F| above every template's |Lf| (-1: unknown)
    // Exact matcher (dice_batch_exact, lazily allocated): per-file result, field masks
    dice::DevBuf<int32_t> d_exact;
    dice::DevBuf<uint64_t> d_fmask;    // [capacity], from whichever of Exact, a text upload and set_rows comes first
    bool fmask_device = false;      // d_fmask holds the last upload's masks (dice_batch_upload_text)
    // dice_batch_upload_text (dice_words.hip): texts, their offsets and lengths, per-file status,
    // counters {overflowed files, long files}
    dice::DevBuf<uint8_t> d_text;
    dice::DevBuf<int64_t> d_toff;
    dice::DevBuf<int32_t> d_tlen;
    dice::DevBuf<uint8_t> d_wstat;
    dice::DevBuf<uint32_t> d_wcnt;
    // dice_batch_content_hash (dice_hash.hip): 0 = the last upload left no text resident, 1 = the
    // texts of dice_batch_upload_text are resident, 2 = and their digests are computed (or queued)
    int32_t text_state = 0;
    // the resident texts are UTF-8 (dice_batch_upload_text_utf8; every other upload clears it): their
    // bytes are content_normalized's, so dice_batch_content_hash flags no file
    bool text_utf8 = false;
    dice::DevBuf<uint8_t> d_hdig;   // [capacity][20] SHA-1 digests
    dice::DevBuf<uint8_t> d_hstat;  // [capacity] 1 = one-byte-per-character text with a byte >= 0x80
    dice::DevBuf<uint32_t> d_hcnt;  // the kernel's next-file counter
    // What has run since the last upload: every upload starts a new epoch, and a match, Exact or
    // project call records the epoch it ran in (dice_batch_projects reads the results of the first two)
    uint32_t epoch = 1, match_epoch = 0, exact_epoch = 0, proj_epoch = 0;
    // dice_batch_projects (dice_project.hip): its inputs on the device (offsets [proj_cap + 1], file
    // flags [capacity], template flags [T]) and one record per project -- license, matched file,
    // distinct licenses, their first proj_k ([P][proj_k]), the matched file's matcher, confidence
    // and digest -- allocated on the first call and grown with the project count
    int64_t proj_cap = 0, proj_P = 0;
    int32_t proj_k = 0;
    bool proj_hash = false;         // the last resolve gathered the digests of dice_batch_content_hash
    dice::DevBuf<int64_t> d_poffs;
    dice::DevBuf<uint8_t> d_pfflags, d_ptflags, d_pdig;
    dice::DevBuf<int32_t> d_plic, d_pmf, d_pnl, d_plist, d_pmatcher;
    dice::DevBuf<double> d_pconf;
    // small-call batch: d_wf/d_len/d_cc/d_rows are views into d_in, the results views into d_out
    dice::DevBytes d_in, d_out;
};

namespace dice {

inline hipStream_t stream_of(dice_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }

// A new upload of n files starts: what the last one left (long-file count, device masks, resident
// texts and their form) is gone, and so is every result (a new epoch).
inline void begin_upload(dice_batch* b, int64_t n) {
    b->n = n;
    b->n_long = 0;
    b->fmask_device = false;
    b->text_state = 0;
    ++b->epoch;
    b->text_utf8 = false;
}

// files with |W_F| above every template's |Lf| (the long-file test of dice_match's routing)
inline int64_t count_long(const dice_ctx* c, const uint32_t* wf, int64_t n) {
    int64_t n_long = 0;
    if (c->prune)
        for (int64_t i = 0; i < n; ++i) n_long += wf[i] > c->prune_max_lf;
    return n_long;
}

inline int check_files(const dice_files* f) {
    if (!f->bits || !f->wordset_size || !f->length || !f->cc_false_positive) return fail(DICE_E_ARG, "NULL file arrays");
    return DICE_OK;
}

}  // namespace dice
