// Template-specialized sparse scoring program for small corpora (T <= 64), gfx950.
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
// large class of them is a byte count (v_and_b32 literal + v_sad_u8) instead of bits, and the
// file's tile is half as long. DICE_PROG_LAYOUT=bits keeps the full-bitset tile. Where it pays
// (plan_mfma), the module also holds the match kernel with the bit region scored on the matrix
// cores (kMfmaPrelude); DICE_PROG_MATCH=valu|mfma overrides the rule.
//
// The source is compiled with hiprtc for gfx950 and cached by hash under the library
// directory (lib/cache/dice_prog_<hash>.co), so a corpus compiles once per machine image.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <sys/stat.h>
#include <unistd.h>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/licensee_dice.h"
#include "dice_program.h"

// dice_ctx / dice_batch internals shared with dice.hip
#include "dice_internal.h"

namespace dice {

namespace {

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
// Overlaps may carry a template index in bits 24-31 (match kernel): only bits 0-23 count.
template <bool FAST>
__device__ __forceinline__ bool ge(u32 oa, i32 da, u32 ob, i32 db) {
    if (FAST) {
#if NARROW_MUL
        // ov < 2^11 and den < 2^21: both products < 2^32, full-rate 24-bit multiplies are exact
        return mul24(oa, (u32)db) >= mul24(ob, (u32)da);
#else
        return (u64)(oa & 0xFFFFFFu) * (u64)(u32)db >= (u64)(ob & 0xFFFFFFu) * (u64)(u32)da;
#endif
    }
    return sc(oa & 0xFFFFFFu, da) >= sc(ob & 0xFFFFFFu, db);
}
#define ACC(d, m) a = __builtin_popcount(f[d] & (m##u)) + a
#define ACCF(d) a = __builtin_popcount(f[d]) + a
)HIP";

// Compact tile only: masked four-byte sum of a count dword (v_and_b32 literal + v_sad_u8 against
// 0, accumulating); the plain-C form serves the host tests.
const char* kCompactPrelude = R"HIP(
#ifndef __HIP_DEVICE_COMPILE__
__device__ __forceinline__ u32 bytesum(u32 x) { return (x & 0xffu) + ((x >> 8) & 0xffu) + ((x >> 16) & 0xffu) + (x >> 24); }
#else
__device__ __forceinline__ u32 bytesum(u32 x) { u32 r; asm("v_sad_u8 %0, %1, 0, 0" : "=v"(r) : "v"(x)); return r; }
#endif
#define ACCS(acc, x, MASK) acc = bytesum((x) & (MASK)) + acc
#define ACCSF1(acc, x) acc = bytesum(x) + acc
)HIP";

const char* kMatchKernel = R"HIP(
extern "C" __global__ __launch_bounds__(64 * WPB MATCH_WAVES) void dice_prog_match(
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
    const u32 wf = wfp[file];
    const i32 lf = lenp[file];
    const bool cc = ccp[file] != 0;
    FILE_PROLOGUE
    const bool fast = CORPUS_FAST && wf < (1u << 20) && lf >= 0 && lf < (1 << 21);
    // running best: bo = template index << 24 | overlap (0xFF: none yet), bd = its denominator
    u32 bo = 0xFF000000u; i32 bd = 1;
    if (__all(fast)) {
        MATCH_BODY(true)
    } else {
        MATCH_BODY(false)
    }
    if (file < n) {
        const i32 bi = (bo >> 24) == 0xFFu ? -1 : (i32)(bo >> 24);
        const u32 bov = bo & 0xFFFFFFu;
        const double s = bi >= 0 ? sc(bov, bd) : 0.0;
        MSTORE(best_out + file, (bi >= 0 && s >= thr) ? bi : -1);
        MSTORE(ov_out + file, bov);
        MSTORE(score_out + file, s);
    }
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
)HIP";

// Matrix kernel template: KM is the compile-time top-k slot count (4 or 16).
const char* kMatrixKernel = R"HIP(
extern "C" __global__ __launch_bounds__(64 * WPB) void KNAME(
    const uint4* __restrict__ files, i64 n, const u32* __restrict__ wfp, const i32* __restrict__ lenp,
    const unsigned char* __restrict__ ccp, i32 k, u32* __restrict__ ov_out, double* __restrict__ score_out,
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
    // template-major [NT][n] outputs: for a fixed template the 64 lanes store contiguously
    u32* orow = ov_out ? ov_out + file : nullptr;
    double* srow = score_out ? score_out + file : nullptr;
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
)HIP";

// Per-template matrix epilogue: store the row entry, then rank-and-shift insertion into the
// KM sorted slots (p = slots that strictly outrank the candidate; a later template goes
// before equal-scored earlier ones, dice.rb:39). Branch-free selects only.
const char* kMatrixOffer = R"HIP(
#define MOFFER(T, CCF)                                                                  \
    {                                                                                   \
        if (valid) { if (orow) MSTORE(orow + (i64)(T) * n, a); if (srow) MSTORE(srow + (i64)(T) * n, sc(a, d)); } \
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
// lane (c, h) is template 32 j + (g & 3) + 8 (g >> 2) + 4 h of file 32 m + c, so one
// v_permlane32_swap of the m = 0 and m = 1 registers leaves lane l with two templates' overlaps
// of file l: no LDS transpose. A workgroup of MWK = 12 waves walks a contiguous share of the tiles,
// wave w taking every MWK-th; the next tile's quads are requested as this tile's K-steps retire
// them. Match mode only: the matrix kernels, bound by their 600 B per file of stores, measured
// 17% slower with the stage and keep the VALU program.
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
// acc[TA] += overlaps of template TA, acc[TB] += of template TB (rows g and g + 4 of the block),
// lane = file: lanes 32-63 of the m = 0 register swap with lanes 0-31 of the m = 1 register
#define MFMA_FOLD2(C0, C1, G, TA, TB) { typedef u32 u32x2_ __attribute__((ext_vector_type(2))); \
    const u32x2_ r_ = __builtin_amdgcn_permlane32_swap((u32)C0[G], (u32)C1[G], false, false); \
    acc[TA] += r_[0]; acc[TB] += r_[1]; }
#define MFMA_FOLD1(C0, C1, G, TA) { typedef u32 u32x2_ __attribute__((ext_vector_type(2))); \
    const u32x2_ r_ = __builtin_amdgcn_permlane32_swap((u32)C0[G], (u32)C1[G], false, false); \
    acc[TA] += r_[0]; }
// Workgroup head: template fragments into LDS, the workgroup's share of the tiles, the wave's first
// tile and its quads
#define MFMA_HEAD \
    __shared__ uint4 tfrag[MFMA_FRAGS * 64]; \
    for (int i = threadIdx.x; i < MFMA_FRAGS * 64; i += 64 * MWK) tfrag[i] = ((const uint4*)dice_mfma_frag)[i]; \
    __syncthreads(); \
    const int lane = threadIdx.x & 63; \
    int ms_ = 0x7F7F7F7F; asm volatile("" : "+v"(ms_)); \
    const i64 nt_ = (n + 63) >> 6; \
    const i64 t1 = nt_ * (i64)(blockIdx.x + 1) / (i64)gridDim.x; \
    i64 tile = nt_ * (i64)blockIdx.x / (i64)gridDim.x + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); \
    if (tile >= t1) return; \
    MFMA_QDECL \
    { const uint4* nq_ = files + tile * (i64)(WQ * 64) + (lane & 31); MFMA_QLOAD }
// Per tile: the quads of the wave's next tile (this one again after the last: loaded, never used)
#define MFMA_TILE \
    const i64 file = tile * 64 + lane; \
    const uint4* fp = files + tile * (i64)(WQ * 64) + lane; \
    const uint4* nq_ = files + (tile + MWK < t1 ? tile + MWK : tile) * (i64)(WQ * 64) + (lane & 31); \
    int ll_ = lane; asm volatile("" : "+v"(ll_));   /* fragment reads stay in the loop (and out of scratch) */
)HIP";

const char* kMatchKernelMfma = R"HIP(
extern "C" __global__ __launch_bounds__(64 * MWK) void dice_prog_match_mfma(
    const uint4* __restrict__ files, i64 n, const u32* __restrict__ wfp, const i32* __restrict__ lenp,
    const unsigned char* __restrict__ ccp, double thr, i32* __restrict__ best_out,
    u32* __restrict__ ov_out, double* __restrict__ score_out) {
    MFMA_HEAD
    for (; tile < t1; tile += MWK) {
        MFMA_TILE
        const u32 wf = wfp[file];
        const i32 lf = lenp[file];
        const bool cc = ccp[file] != 0;
        FILE_PROLOGUE_MFMA
        const bool fast = CORPUS_FAST && wf < (1u << 20) && lf >= 0 && lf < (1 << 21);
        u32 bo = 0xFF000000u; i32 bd = 1;
        if (__all(fast)) {
            MATCH_BODY(true)
        } else {
            MATCH_BODY(false)
        }
        if (file < n) {
            const i32 bi = (bo >> 24) == 0xFFu ? -1 : (i32)(bo >> 24);
            const u32 bov = bo & 0xFFFFFFu;
            const double s = bi >= 0 ? sc(bov, bd) : 0.0;
            MSTORE(best_out + file, (bi >= 0 && s >= thr) ? bi : -1);
            MSTORE(ov_out + file, bov);
            MSTORE(score_out + file, s);
        }
    }
}
)HIP";

uint64_t fnv1a(const std::string& s) {
    uint64_t h = 1469598103934665603ULL;
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ULL;
    }
    return h;
}

std::string lib_dir() {
    Dl_info info;
    if (dladdr((void*)&fnv1a, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t s = p.rfind('/');
        if (s != std::string::npos) return p.substr(0, s);
    }
    return ".";
}

std::string cache_dir() {
    const char* env = getenv("DICE_CACHE_DIR");
    std::string d = env && *env ? std::string(env) : lib_dir() + "/cache";
    mkdir(d.c_str(), 0755);
    return d;
}

bool read_file(const std::string& path, std::vector<char>& out) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    out.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    return !out.empty();
}

}  // namespace

// Build the entry list (template-major, dword ascending) from the template bitsets.
static void build_entries(const dice_templates* t, int32_t w64, Program& p) {
    p.prog.clear();
    const int32_t w32 = w64 * 2;
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(t->lf_bits + (size_t)i * w64);
        for (int32_t d = 0; d < w32; ++d)
            if (row[d]) p.prog.push_back(Entry{i, d, row[d]});
    }
}

// One dword-major accumulation statement (plain C; ACC_C_ONLY of acc_block).
static std::string acc_stmt(const Entry& en) {
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
static std::string acc_block(const std::vector<Entry>& dm, size_t b, size_t e) {
    std::vector<int32_t> tpls;
    std::vector<int> fk;
    for (size_t i = b; i < e; ++i) {
        if (std::find(tpls.begin(), tpls.end(), dm[i].tpl) == tpls.end()) tpls.push_back(dm[i].tpl);
        const int k = dm[i].dword % 4;
        if (std::find(fk.begin(), fk.end(), k) == fk.end()) fk.push_back(k);
    }
    auto acc_op = [&](int32_t tpl) { return (int)(std::find(tpls.begin(), tpls.end(), tpl) - tpls.begin()); };
    // 4 temporaries: the v_and of up to 4 entries issue back to back, then their v_bcnt, so
    // no v_bcnt waits on the v_and right before it
    constexpr int kTmp = 4;
    const int tmp0 = (int)tpls.size();
    auto f_op = [&](int k) { return tmp0 + kTmp + (int)(std::find(fk.begin(), fk.end(), k) - fk.begin()); };
    std::ostringstream a, c;
    a << "ACC_ASM_ONLY(asm(\"";
    bool first = true;
    auto emit = [&](const std::string& ins) {
        if (!first) a << "\\n\\t";
        a << ins;
        first = false;
    };
    for (size_t g = b; g < e; g += kTmp) {
        const size_t ge = std::min(e, g + kTmp);
        for (size_t i = g; i < ge; ++i) {
            const Entry& en = dm[i];
            if (en.mask == 0xFFFFFFFFu) continue;
            std::ostringstream ins;
            ins << "v_and_b32 %" << tmp0 + (int)(i - g) << ", 0x" << std::hex << en.mask << std::dec << ", %"
                << f_op(en.dword % 4);
            emit(ins.str());
        }
        for (size_t i = g; i < ge; ++i) {
            const Entry& en = dm[i];
            std::ostringstream ins;
            const int src = en.mask == 0xFFFFFFFFu ? f_op(en.dword % 4) : tmp0 + (int)(i - g);
            if (en.sum)   // count dword: sum of the selected bytes
                ins << "v_sad_u8 %" << acc_op(en.tpl) << ", %" << src << ", 0, %" << acc_op(en.tpl);
            else
                ins << "v_bcnt_u32_b32 %" << acc_op(en.tpl) << ", %" << src << ", %" << acc_op(en.tpl);
            emit(ins.str());
        }
        for (size_t i = g; i < ge; ++i) c << acc_stmt(dm[i]);
    }
    a << "\" : ";
    for (size_t i = 0; i < tpls.size(); ++i) a << "\"+v\"(acc[" << tpls[i] << "]), ";
    for (int k = 0; k < kTmp; ++k) a << "\"=&v\"(t_[" << k << "])" << (k + 1 < kTmp ? ", " : "");
    a << " : ";
    for (size_t i = 0; i < fk.size(); ++i) a << (i ? ", " : "") << "\"v\"(f[" << fk[i] << "])";
    a << ");)";
    std::string cs = c.str();
    std::replace(cs.begin(), cs.end(), '\n', ' ');
    return "{ u32 t_[4]; " + a.str() + " ACC_C_ONLY(" + cs + ") (void)t_; }\n";
}

// Accumulations of one quad, in blocks of at most kAccBlock entries.
static std::string acc_quad(const std::vector<Entry>& dm, size_t b0, size_t end, int32_t q) {
    constexpr size_t kAccBlock = 4;   // entries per asm block (2 and 8 measured slower)
    std::string out;
    const char* diag = diag_env("DICE_PROG_DIAG");   // diagnostics only: results are wrong
    if (diag && strcmp(diag, "noacc") == 0) return "acc[" + std::to_string(q) + " % NT] ^= f[0] ^ f[1] ^ f[2] ^ f[3];\n";
    for (size_t b = b0; b < end; b += kAccBlock) out += acc_block(dm, b, std::min(end, b + kAccBlock));
    return out;
}


// Emits `text` as the body of a one-line-per-statement macro.
static void emit_macro(std::ostringstream& s, const std::string& head, const std::string& text) {
    s << "#define " << head << " \\\n";
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) s << line << " \\\n";
    s << "\n";
}

// Cost rule of the matrix-core stage: it runs when the VALU instructions of the bit entries exceed
// kMfmaPayRatio times the stage's own cost in the same unit (one VALU issue = 4 cycles: widening 5
// per fragment, ~3 per template to fold, matrix cycles / 4). One measured point: the vendored corpus,
// ratio 2.02, gains 1.21x. The constant sits halfway between break-even on
// paper and that point; it is not calibrated on a second corpus.
constexpr double kMfmaPayRatio = 1.5;
constexpr int kMfmaMatchWaves = 12;   // MWK of the generated kernel
constexpr int64_t kMfmaMaxFragBytes = 96 * 1024;   // one 12-wave workgroup per CU: 3 waves per SIMD

// Shape and costs of the stage for the layout in p (no slot order needed).
static void plan_mfma(const dice_templates* t, Program& p) {
    MfmaTables& m = p.mf;
    const CompactLayout& L = p.layout;
    const int32_t qb = (L.bit_dwords + 3) / 4, np = (qb + 1) / 2;
    m.ksteps = 4 * np;
    m.ntiles = (t->n_templates + 31) / 32;
    m.valu_cost = 0;
    for (const Entry& e : p.prog)
        if (!e.sum) m.valu_cost += e.mask == 0xFFFFFFFFu ? 1 : 2;
    m.stage_cost = 2 * 5 * (int64_t)m.ksteps + 3 * (int64_t)t->n_templates + (int64_t)m.ksteps * m.ntiles * 2 * 32 / 4;
    m.eligible = L.bit_dwords > 0 && (int64_t)m.ksteps * m.ntiles * 1024 <= kMfmaMaxFragBytes;
    m.pays = m.eligible && (double)m.valu_cost > kMfmaPayRatio * (double)m.stage_cost;
}

// Fragment table and file-side map, once p.qperm is known.
static void build_mfma_tables(const dice_templates* t, Program& p) {
    MfmaTables& m = p.mf;
    const CompactLayout& L = p.layout;
    const int32_t T = t->n_templates, qb = (L.bit_dwords + 3) / 4, np = m.ksteps / 4;
    std::vector<int32_t> slot_of((size_t)L.quads, 0);
    for (size_t s = 0; s < p.qperm.size(); ++s) slot_of[(size_t)p.qperm[s]] = (int32_t)s;
    m.slots.assign((size_t)2 * np, -1);
    for (int32_t q = 0; q < qb; ++q) m.slots[(size_t)q] = slot_of[(size_t)q];
    std::vector<uint32_t> mask((size_t)T * std::max(1, L.bit_dwords), 0u);
    for (const Entry& e : p.prog)
        if (!e.sum) mask[(size_t)e.tpl * L.bit_dwords + e.dword] = e.mask;
    m.frag.assign((size_t)m.ksteps * m.ntiles * 64 * 4, 0u);
    m.map.assign((size_t)m.ksteps * 64, -1);
    for (int32_t s = 0; s < m.ksteps; ++s) {
        for (int32_t h = 0; h < 2; ++h) {
            const int32_t q = 2 * (s / 4) + h, dw = 4 * q + s % 4;
            if (q >= qb || dw >= L.bit_dwords) continue;
            const int32_t tile_dword = 4 * m.slots[(size_t)q] + s % 4;
            for (int32_t e = 0; e < 32; ++e) {   // element e = 8 k + i: nibble i of fragment dword k, bit 4 i + k
                const int32_t bit = 4 * (e % 8) + e / 8;
                if (32 * dw + bit < L.n_bits) m.map[(size_t)s * 64 + 32 * h + e] = 32 * tile_dword + bit;
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
}

// Program order: dword-major -- every template accumulator stays live (acc[NT]); file quads are
// loaded in bursts right before they are consumed, so a file dword's live range is a few
// instructions; the epilogue (denominator, compare) runs once per template after the last quad.
// (The template-major order, the whole bitset loaded up front and each template retired in turn,
// measured 2% slower and is retired: DESIGN.md Appendix B.)
// `wq` is the tile's quad count; `burst` the quads per load group.
std::string program_source(const dice_templates* t, Program& p, int32_t wq, bool corpus_fast, int burst = 5) {
    std::ostringstream s;
    s << "#define WPB " << p.wpb << "\n";
    s << "// dice sparse program: T=" << t->n_templates << " V=" << t->n_vocab << " entries=" << p.prog.size()
      << " order=d\n";
    if (p.compact)
        s << "// layout=compact threshold=" << p.layout.threshold << " bits=" << p.layout.n_bits
          << " bit_dwords=" << p.layout.bit_dwords << " count_bytes=" << p.layout.n_fields << " burst=" << burst << "\n";
    s << "#define MATCH_WAVES \n";
    uint32_t max_lf = 0;
    for (int32_t i = 0; i < t->n_templates; ++i) max_lf = std::max(max_lf, t->lf_size[i]);
    // v_and/v_bcnt as asm blocks (ACC_ASM; host tests compile the plain-C form), non-temporal file
    // loads (FILE_NT) and outputs (OUT_NT: written once, never re-read; config 5 -1.9%, 3 reps)
    s << "#define ACC_ASM 1\n";
    s << "#define FILE_NT 1\n";
    s << "#define OUT_NT 1\n";
    s << "#define WQ " << wq << "\n#define NT " << t->n_templates << "\n#define CORPUS_FAST "
      << (corpus_fast ? 1 : 0) << "\n#define NARROW_MUL " << (max_lf < (1u << 11) ? 1 : 0) << "\n" << kPrelude;
    if (p.compact) s << kCompactPrelude;

    std::vector<std::string> den(t->n_templates);
    for (int32_t i = 0; i < t->n_templates; ++i) {
        const int32_t base = (int32_t)t->lf_size[i] - (int32_t)t->fields_set_size[i];
        std::ostringstream d;
        d << "d = dn(" << base << ", " << t->length_slack[i] << ", " << t->length[i] << ", wf, lf); ";
        den[i] = d.str();
    }
    auto offer = [&](int32_t i) {
        std::ostringstream o;
        if (t->is_cc[i]) o << "if (!cc) ";
        // a carries the template index in its top byte (ACC_INIT): one select moves index and
        // overlap together; v_mul_u32_u24 reads only the low 24 bits (the overlap)
        o << "{ if ((!FASTV && (bo >> 24) == 0xFFu) || ge<FASTV>(a, d, bo, bd)) { bo = a; bd = d; } }";
        return o.str();
    };
    std::ostringstream match_body, matrix_body, prologue, mfma_pro, mfma_defs;
    {
        std::vector<Entry> dm(p.prog);
        std::stable_sort(dm.begin(), dm.end(), [](const Entry& x, const Entry& y) {
            return x.dword != y.dword ? x.dword < y.dword : x.tpl < y.tpl;
        });
        prologue << "u32 acc[NT];\n_Pragma(\"unroll\") for (int i = 0; i < NT; ++i) acc[i] = ACC_INIT(i);\n";
        // quads the program touches, their entry ranges in dm and their VALU cost
        std::vector<int32_t> quads;
        std::vector<std::pair<size_t, size_t>> range;   // [begin, end) in dm, per quads[] slot
        std::vector<int> cost;
        for (size_t i = 0; i < dm.size(); ++i) {
            if (quads.empty() || quads.back() != dm[i].dword / 4) {
                quads.push_back(dm[i].dword / 4);
                range.push_back({i, i});
                cost.push_back(0);
            }
            range.back().second = i + 1;
            cost.back() += dm[i].mask == 0xFFFFFFFFu ? 1 : 2;
        }
        {   // processing order: alternating costliest and cheapest quads, which spreads the VALU
            // work evenly over the stream (the packed vocabulary puts the widely shared words --
            // 120-250 VALU per quad -- at the end, the rare ones at 4-40 first): -5.5% config 2 vs
            // memory order (costliest-first -4.4%, equal VALU per burst +-0)
            std::vector<size_t> idx(quads.size());
            for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
            {
                std::vector<size_t> z;
                for (size_t lo = 0, hi = idx.size(); lo < hi;) {
                    z.push_back(idx[lo++]);
                    if (lo < hi) z.push_back(idx[--hi]);
                }
                idx.swap(z);
            }
            std::vector<int32_t> q2;
            std::vector<std::pair<size_t, size_t>> r2;
            for (size_t i : idx) {
                q2.push_back(quads[i]);
                r2.push_back(range[i]);
            }
            quads.swap(q2);
            range.swap(r2);
        }
        // Tile layout in processing order: tile slot i holds the vocabulary quad processed i-th
        // (dice_pack_tiles applies p.qperm), so a wave's loads walk its 28 KiB tile front to back
        // while the VALU work stays zipped.
        {
            p.qperm.clear();
            std::vector<char> seen((size_t)wq, 0);
            for (int32_t q : quads) {
                p.qperm.push_back(q);
                seen[(size_t)q] = 1;
            }
            for (int32_t q = 0; q < wq; ++q)
                if (!seen[(size_t)q]) p.qperm.push_back(q);   // quads no template reads (never loaded)
            for (size_t i = 0; i < quads.size(); ++i) quads[i] = (int32_t)i;
            s << "// QPERM";
            for (int32_t q : p.qperm) s << " " << q;
            s << "\n";
        }
        {
            // bursts: quads in groups of `nb` = 5, double-buffered in register sets p0_* / p1_*;
            // group g+1 is requested (nb contiguous 1 KiB wave loads back to back) before group g
            // is consumed. With non-temporal loads, bursts of 3 measured ~1.5% ahead of an 8-deep
            // ring at 92 instead of 124 VGPRs, 4 another ~3.5%, 5 another 1.8% (6: -0.3%)
            const int nb = std::max(1, std::min<int>(burst, (int)quads.size()));
            const size_t ng = (quads.size() + nb - 1) / nb;
            auto group_loads = [&](std::ostringstream& o, size_t g, int set) {
                for (size_t i = g * nb; i < std::min(quads.size(), (g + 1) * nb); ++i)
                    o << "p" << set << "_" << (i - g * nb) << " = ldq(fp + " << quads[i] * 64 << "); ";
                o << "\n";
            };
            auto stream = [&](std::ostringstream& o) {
                for (size_t g = 0; g < ng; ++g) {
                    const int cur = (int)(g % 2), nxt = 1 - cur;
                    o << "__builtin_amdgcn_sched_barrier(0);\n";
                    if (g + 1 < ng) group_loads(o, g + 1, nxt);
                    o << "__builtin_amdgcn_sched_barrier(0);\n";
                    for (size_t i = g * nb; i < std::min(quads.size(), (g + 1) * nb); ++i) {
                        o << "{ const uint4 v = p" << cur << "_" << (i - g * nb) << "; const u32 f[4] = {v.x, v.y, v.z, v.w};\n";
                        o << acc_quad(dm, range[i].first, range[i].second, quads[i]);
                        o << "}\n";
                    }
                }
            };
            std::ostringstream decl;
            for (int i = 0; i < nb; ++i) decl << "uint4 p0_" << i << ", p1_" << i << ";\n";
            prologue << decl.str();
            group_loads(prologue, 0, 0);
            stream(prologue);
        }
        if (p.compact && p.mf.eligible) build_mfma_tables(t, p);
        if (p.mfma) {
            // the matrix-core form of the prologue (kMfmaPrelude): count quads requested lane per
            // file, the K-steps pair by pair of bit quads with the next tile's pair requested
            // behind them, the fold into acc[], then the count entries as in the VALU program
            const MfmaTables& m = p.mf;
            const int32_t np = m.ksteps / 4, nj = m.ntiles, T = t->n_templates;
            std::ostringstream& o = mfma_pro;
            o << "u32 acc[NT];\n_Pragma(\"unroll\") for (int i = 0; i < NT; ++i) acc[i] = ACC_INIT(i);\n";
            std::vector<std::pair<size_t, size_t>> crange(quads.size(), {0, 0});   // count entries per slot
            for (size_t i = 0; i < quads.size(); ++i) {
                size_t b = range[i].first;
                while (b < range[i].second && !dm[b].sum) ++b;
                crange[i] = {b, range[i].second};
                if (b < range[i].second) o << "const uint4 cq_" << i << " = ldq(fp + " << quads[i] * 64 << ");\n";
            }
            for (int32_t j = 0; j < nj; ++j) o << "v16f c" << j << "_0 = {}, c" << j << "_1 = {};\n";
            const char* comp = "xyzw";
            for (int32_t u = 0; u < np; ++u) {
                for (int32_t d = 0; d < 4; ++d) {
                    const int32_t s = 4 * u + d;
                    bool any = false;
                    for (int32_t e = 0; e < 64; ++e) any = any || m.map[(size_t)s * 64 + e] >= 0;
                    if (!any) continue;
                    o << "{ const v8i b0_ = widen_a(q0_" << u << "." << comp[d] << "), b1_ = widen_a(q1_" << u << "."
                      << comp[d] << ");\n";
                    for (int32_t j = 0; j < nj; ++j)
                        o << "{ const v8i a_ = frag8(tfrag[" << (s * nj + j) * 64 << " + ll_]); c" << j << "_0 = MFMA44(a_, b0_, c"
                          << j << "_0); c" << j << "_1 = MFMA44(a_, b1_, c" << j << "_1); }\n";
                    o << "}\n";
                }
                o << "q0_" << u << " = ldq(nq_ + o_" << u << "); q1_" << u << " = ldq(nq_ + o_" << u << " + 32);\n";
            }
            for (int32_t j = 0; j < nj; ++j)
                for (int32_t g = 0; g < 16; ++g) {
                    const int32_t ta = 32 * j + (g & 3) + 8 * (g >> 2), tb = ta + 4;
                    if (ta >= T) continue;
                    if (tb < T)
                        o << "MFMA_FOLD2(c" << j << "_0, c" << j << "_1, " << g << ", " << ta << ", " << tb << ")\n";
                    else
                        o << "MFMA_FOLD1(c" << j << "_0, c" << j << "_1, " << g << ", " << ta << ")\n";
                }
            for (size_t i = 0; i < quads.size(); ++i) {
                if (crange[i].first == crange[i].second) continue;
                o << "{ const u32 f[4] = {cq_" << i << ".x, cq_" << i << ".y, cq_" << i << ".z, cq_" << i << ".w};\n";
                o << acc_quad(dm, crange[i].first, crange[i].second, quads[i]);
                o << "}\n";
            }
            // per-lane quad offsets (lane half h takes the odd quad of each pair), declarations, loads
            std::ostringstream qd, ql;
            for (int32_t u = 0; u < np; ++u) {
                const int32_t s0 = m.slots[(size_t)2 * u], s1 = m.slots[(size_t)2 * u + 1] >= 0 ? m.slots[(size_t)2 * u + 1] : s0;
                qd << "const int o_" << u << " = (lane >> 5) ? " << s1 * 64 << " : " << s0 * 64 << "; uint4 q0_" << u
                   << ", q1_" << u << ";\n";
                ql << "q0_" << u << " = ldq(nq_ + o_" << u << "); q1_" << u << " = ldq(nq_ + o_" << u << " + 32);\n";
            }
            emit_macro(mfma_defs, "MFMA_QDECL", qd.str());
            emit_macro(mfma_defs, "MFMA_QLOAD", ql.str());
        }
        for (int32_t i = 0; i < t->n_templates; ++i) {
            match_body << "{ const u32 a = acc[" << i << "]; i32 d; " << den[i] << offer(i) << " }\n";
            matrix_body << "{ const u32 a = acc[" << i << "]; i32 d; " << den[i] << "MOFFER(" << i << ", "
                        << (t->is_cc[i] ? 1 : 0) << ") }\n";
        }
    }
    emit_macro(s, "FILE_PROLOGUE", prologue.str());
    const char* diag = diag_env("DICE_PROG_DIAG");   // diagnostics only: results are wrong
    s << "#define WAVE_TIMING " << (diag && strcmp(diag, "timing") == 0 ? 1 : 0) << "\n";
    if (diag && strcmp(diag, "noepi") == 0) {
        std::ostringstream mb;
        mb << "bd = 1; bo = 0; _Pragma(\"unroll\") for (int i = 0; i < NT; ++i) bo += acc[i];\n";
        match_body.str(mb.str());
    }
    emit_macro(s, "MATCH_BODY(FASTV_) { constexpr bool FASTV = FASTV_;", match_body.str() + "}");
    s << "#define ACC_INIT(i) ((u32)(i) << 24)\n" << kMatchKernel
      << "#undef ACC_INIT\n#define ACC_INIT(i) 0u\n";
    s << kMatrixOffer;
    emit_macro(s, "MATRIX_BODY(FASTV_) { constexpr bool FASTV = FASTV_;", matrix_body.str() + "}");
    for (int km : {4, 16}) {
        s << "#define KM " << km << "\n#define KNAME dice_prog_matrix" << km << "\n" << kMatrixKernel
          << "#undef KM\n#undef KNAME\n";
    }
    if (p.mfma) {
        // the match kernel with the matrix-core accumulate stage, device compile only
        s << "#ifdef __HIP_DEVICE_COMPILE__\n#define MFMA_FRAGS " << p.mf.ksteps * p.mf.ntiles << "\n";
        s << "__device__ const u32 dice_mfma_frag[" << p.mf.frag.size() << "] __attribute__((aligned(16))) = {\n" << std::hex;
        for (size_t i = 0; i < p.mf.frag.size(); ++i) s << "0x" << p.mf.frag[i] << (i % 16 == 15 ? ",\n" : ",");
        s << std::dec << "};\n" << kMfmaPrelude << mfma_defs.str();
        emit_macro(s, "FILE_PROLOGUE_MFMA", mfma_pro.str());
        s << "#define MWK " << kMfmaMatchWaves << "\n#undef ACC_INIT\n#define ACC_INIT(i) ((u32)(i) << 24)\n" << kMatchKernelMfma
          << "#undef ACC_INIT\n#define ACC_INIT(i) 0u\n#endif\n";
    }
    return s.str();
}

// Compile (or find in the cache) the code object for `src`. No device needed.
static int compile_cached(const std::string& src, std::vector<char>& code, std::string* path_out) {
    const uint64_t h = fnv1a(src);
    char name[64];
    snprintf(name, sizeof(name), "dice_prog_%016llx.co", (unsigned long long)h);
    const std::string path = cache_dir() + "/" + name;
    if (!read_file(path, code)) {
        hiprtcProgram prog;
        if (hiprtcCreateProgram(&prog, src.c_str(), "dice_prog.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
            return fail(DICE_E_DEVICE, "hiprtcCreateProgram failed");
        const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
        hiprtcResult r = hiprtcCompileProgram(prog, 3, opts);
        if (r != HIPRTC_SUCCESS) {
            size_t ls = 0;
            hiprtcGetProgramLogSize(prog, &ls);
            std::string log(ls, '\0');
            if (ls) hiprtcGetProgramLog(prog, &log[0]);
            hiprtcDestroyProgram(&prog);
            return fail(DICE_E_DEVICE, "hiprtc compile failed: " + log.substr(0, 2000));
        }
        size_t cs = 0;
        hiprtcGetCodeSize(prog, &cs);
        code.resize(cs);
        hiprtcGetCode(prog, code.data());
        hiprtcDestroyProgram(&prog);
        // best-effort cache write (atomic rename)
        const std::string tmp = path + ".tmp." + std::to_string(getpid());
        {
            std::ofstream out(tmp, std::ios::binary);
            if (out) out.write(code.data(), (std::streamsize)code.size());
        }
        rename(tmp.c_str(), path.c_str());
    }
    if (path_out) *path_out = path;
    return DICE_OK;
}

static int compile_or_load(dice_ctx* c, const std::string& src) {
    std::vector<char> code;
    int rc = compile_cached(src, code, nullptr);
    if (rc != DICE_OK) return rc;
    if (hipModuleLoadData(&c->module, code.data()) != hipSuccess) return fail(DICE_E_DEVICE, "hipModuleLoadData failed");
    if (hipModuleGetFunction(&c->prog_match, c->module, "dice_prog_match") != hipSuccess ||
        hipModuleGetFunction(&c->prog_matrix, c->module, "dice_prog_matrix4") != hipSuccess ||
        hipModuleGetFunction(&c->prog_matrix16, c->module, "dice_prog_matrix16") != hipSuccess)
        return fail(DICE_E_DEVICE, "hipModuleGetFunction failed");
    if (c->prog.mfma) {
        if (hipModuleGetFunction(&c->prog_match_mfma, c->module, "dice_prog_match_mfma") != hipSuccess)
            return fail(DICE_E_DEVICE, "hipModuleGetFunction failed");
        if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->n_cu < 1)
            c->n_cu = 256;
    }
    return DICE_OK;
}

// The matrix-core kernels take a launch when the module has them and the batch gives every CU a
// tile (below that the fragment fill per workgroup outweighs the stage; DICE_PROG_MATCH=mfma
// takes them at every size). One workgroup per CU at most, never more than there are tiles.
static bool mfma_launch(const dice_ctx* c, int64_t n_tiles, unsigned* grid) {
    if (!c->prog.mfma || !(c->prog.mfma_forced || n_tiles >= c->n_cu)) return false;
    *grid = (unsigned)std::min<int64_t>(n_tiles, c->n_cu);
    return true;
}

static bool corpus_in_fast_envelope(const dice_templates* t) {
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

static std::string source_for(const dice_templates* t, Program& prog) {
    const int32_t w64 = (t->n_vocab + 63) / 64;
    build_entries(t, w64, prog);
    prog.wpb = 4;   // waves per workgroup (1, 2 and 8 within +-1.5%)
    return program_source(t, prog, (w64 + 1) / 2, corpus_in_fast_envelope(t));
}

// ---------------------------------------------------------------------------------------
// Compact tile: layout derivation, its program entries and the repack tables
// ---------------------------------------------------------------------------------------

// Template-membership column of every vocabulary word (bit i: the word is in template i).
static std::vector<uint64_t> word_columns(const dice_templates* t) {
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
static void place_words(const std::vector<WordClass>& classes, int32_t V, int32_t th, CompactLayout& L) {
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
static void build_compact_entries(const dice_templates* t, const std::vector<uint64_t>& col, const CompactLayout& L,
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

static int64_t entry_cost(const std::vector<Entry>& es) {
    int64_t c = 0;
    for (const Entry& e : es) c += e.mask == 0xFFFFFFFFu ? 1 : 2;
    return c;
}

// Layout for the corpus: the class-size threshold that gives the fewest tile quads, on a tie the
// fewest program instructions (then the smallest threshold). A class of <= 8 words never takes
// more bits as bits than as a count byte, so thresholds start at 8.
static void derive_layout(const dice_templates* t, CompactLayout& best, std::vector<Entry>& entries) {
    const int32_t V = t->n_vocab;
    const std::vector<uint64_t> col = word_columns(t);
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
        const int64_t cost = entry_cost(es);
        if (!have || L.quads < best.quads || (L.quads == best.quads && cost < best_cost)) {
            best = std::move(L);
            entries.swap(es);
            best_cost = cost;
            have = true;
        }
    }
}

// Repack pieces for dice_pack_compact, per tile dword in slot order (p.qperm applied).
static void build_pack_lists(Program& p, int32_t V) {
    const CompactLayout& L = p.layout;
    std::vector<int32_t> slot_of((size_t)L.quads, 0);
    for (size_t s = 0; s < p.qperm.size(); ++s) slot_of[(size_t)p.qperm[s]] = (int32_t)s;
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
    p.pack_lists.assign((size_t)L.quads * 4, {});
    for (size_t i = 0; i < ps.size(); ++i) {
        const Key& k = ps[i].first;
        std::vector<PackPiece>& l = p.pack_lists[(size_t)k.dst];
        if (i && !(ps[i - 1].first < k))   // same (dst, src, op): one piece
            l.back().mask |= ps[i].second;
        else
            l.push_back(PackPiece{k.src, ps[i].second, k.op});
    }
}

// The repack kernel of the compact tile, generated beside the program (device compile only: the
// host tests pack their tiles in numpy). One workgroup per 64-file tile stages the tile's rows
// through LDS with coalesced 8-byte loads (row stride odd in dwords, so the 64 lanes of a wave,
// one file each, hit distinct banks; rows too long for 64 KiB are read from global memory
// instead), then each of its four waves builds whole quads -- row dwords at constant LDS
// offsets, masks and shifts as literals -- and stores one uint4 per lane. Quads are dealt to
// the waves by piece count, largest first.
static std::string pack_source(const Program& p, int32_t w64) {
    const CompactLayout& L = p.layout;
    int32_t stride = (2 * w64) | 1;
    if ((size_t)64 * stride * 4 > 64 * 1024) stride = 0;
    std::ostringstream s;
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
    return s.str();
}

static std::string compact_source_for(const dice_templates* t, Program& prog) {
    prog.compact = true;
    derive_layout(t, prog.layout, prog.prog);
    prog.wpb = 4;
    // DICE_PROG_MATCH (read at dice_create): `mfma` takes the matrix-core stage wherever it is
    // eligible, `valu` never; by default the cost rule decides
    plan_mfma(t, prog);
    const char* pm = getenv("DICE_PROG_MATCH");
    prog.mfma_forced = pm && strcmp(pm, "mfma") == 0 && prog.mf.eligible;
    prog.mfma = prog.mfma_forced || (!(pm && strcmp(pm, "valu") == 0) && prog.mf.pays);
    // bursts of 5 quads as for the full-bitset tile (3, 4, 5 and 7 measure alike on 14 quads)
    const std::string src = program_source(t, prog, prog.layout.quads, corpus_in_fast_envelope(t));
    build_pack_lists(prog, t->n_vocab);
    return src + pack_source(prog, (t->n_vocab + 63) / 64);
}

// DICE_PROG_LAYOUT=bits (read at dice_create) keeps the full-bitset tile: fallback and A/B leg.
static bool compact_wanted() {
    const char* e = getenv("DICE_PROG_LAYOUT");
    return !(e && strcmp(e, "bits") == 0);
}

bool program_wanted(const dice_templates* t) {
    const char* force = getenv("DICE_FORCE_DENSE");
    return !(force && *force == '1') && t->n_templates <= kProgramMaxTemplates;
}

int program_setup(dice_ctx* c, const dice_templates* t) {
    c->kind = 0;
    c->twq = c->wq;
    if (!program_wanted(t)) return DICE_OK;
    if (compact_wanted()) {
        const std::string src = compact_source_for(t, c->prog);
        int rc = compile_or_load(c, src);
        if (rc != DICE_OK) return rc;
        const Program& p = c->prog;
        if (p.qperm.size() != (size_t)p.layout.quads) return fail(DICE_E_STATE, "program tile permutation size");
        if (hipModuleGetFunction(&c->prog_pack, c->module, "dice_pack_compact") != hipSuccess)
            return fail(DICE_E_DEVICE, "hipModuleGetFunction failed");
        c->twq = p.layout.quads;
        c->kind = 1;
        return DICE_OK;
    }
    const std::string src = source_for(t, c->prog);
    int rc = compile_or_load(c, src);
    if (rc != DICE_OK) return rc;
    if (!c->prog.qperm.empty()) {
        const size_t bytes = c->prog.qperm.size() * sizeof(int32_t);
        if (c->prog.qperm.size() != (size_t)c->wq) return fail(DICE_E_STATE, "program tile permutation size");
        if ((rc = dalloc_bytes(reinterpret_cast<void**>(&c->d_qperm), bytes)) != DICE_OK) return rc;
        if (hipMemcpy(c->d_qperm, c->prog.qperm.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(DICE_E_DEVICE, "program tile permutation upload failed");
    }
    c->kind = 1;
    return DICE_OK;
}

int program_launch_pack(dice_ctx* c, dice_batch* b, int64_t n, hipStream_t s) {
    const int64_t n_tiles = (n + 63) / 64;
    if (n_tiles == 0) return DICE_OK;
    void* args[] = {&b->d_rows, &n, &b->d_tiles};
    if (hipModuleLaunchKernel(c->prog_pack, (unsigned)n_tiles, 1, 1, 256, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_pack_compact failed");
    return DICE_OK;
}

int program_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s) {
    const int64_t n_tiles = (b->n + 63) / 64;
    const int32_t wpb = c->prog.wpb;
    unsigned grid = (unsigned)((n_tiles + wpb - 1) / wpb), threads = 64 * wpb;
    hipFunction_t fn = c->prog_match;
    if (mfma_launch(c, n_tiles, &grid)) {
        fn = c->prog_match_mfma;
        threads = 64 * kMfmaMatchWaves;
    }
    int64_t n = b->n;
    void* args[] = {&b->d_tiles, &n, &b->d_wf, &b->d_len, &b->d_cc, &thr, &b->d_best, &b->d_ov, &b->d_score};
    if (hipModuleLaunchKernel(fn, grid, 1, 1, threads, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_prog_match failed");
    return DICE_OK;
}

int program_launch_matrix(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s) {
    const int64_t n_tiles = (b->n + 63) / 64;
    const int32_t wpb = c->prog.wpb;
    const unsigned grid = (unsigned)((n_tiles + wpb - 1) / wpb);
    int64_t n = b->n;
    int32_t kk = k;
    int32_t* tki = k > 0 ? b->d_tki : nullptr;
    double* tks = k > 0 ? b->d_tks : nullptr;
    void* args[] = {&b->d_tiles, &n, &b->d_wf, &b->d_len, &b->d_cc, &kk, &b->d_mov, &b->d_mscore, &tki, &tks};
    hipFunction_t fn = k <= 4 ? c->prog_matrix : c->prog_matrix16;
    if (hipModuleLaunchKernel(fn, grid, 1, 1, 64 * wpb, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_prog_matrix failed");
    return DICE_OK;
}

}  // namespace dice

extern "C" int dice_precompile(const dice_templates* t, char* path, int32_t path_cap) {
    if (!t || t->n_templates < 1 || t->n_vocab < 1 || !t->lf_bits) return dice::fail(DICE_E_ARG, "invalid dice_templates");
    if (!dice::program_wanted(t)) return dice::fail(DICE_E_STATE, "corpus uses the dense kernel");
    // both layouts, so the DICE_PROG_LAYOUT=bits leg finds its code object too; the path
    // written is the one dice_create will load
    std::string p[2];
    for (int compact = 0; compact < 2; ++compact) {
        dice::Program prog;
        const std::string src = compact ? dice::compact_source_for(t, prog) : dice::source_for(t, prog);
        std::vector<char> code;
        int rc = dice::compile_cached(src, code, &p[compact]);
        if (rc != DICE_OK) return rc;
    }
    if (path && path_cap > 0) snprintf(path, (size_t)path_cap, "%s", p[dice::compact_wanted() ? 1 : 0].c_str());
    return DICE_OK;
}

extern "C" int64_t dice_program_source_compact(const dice_templates* t, char* buf, int64_t cap) {
    if (!t || t->n_templates < 1 || t->n_vocab < 1 || !t->lf_bits || t->n_templates > dice::kProgramMaxTemplates)
        return -1;
    dice::Program prog;
    const std::string src = dice::compact_source_for(t, prog);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, src.size());
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return (int64_t)src.size();
}

extern "C" int32_t dice_program_layout(const dice_templates* t, int32_t* dest, int32_t* count_base, int32_t* qperm,
                                       int32_t qperm_cap) {
    if (!t || t->n_templates < 1 || t->n_vocab < 1 || !t->lf_bits || t->n_templates > dice::kProgramMaxTemplates)
        return -1;
    dice::Program prog;
    (void)dice::compact_source_for(t, prog);
    const dice::CompactLayout& L = prog.layout;
    if (dest) memcpy(dest, L.dest.data(), L.dest.size() * sizeof(int32_t));
    if (count_base) *count_base = 4 * L.bit_dwords;
    if (qperm) {
        if (qperm_cap < L.quads) return -1;
        memcpy(qperm, prog.qperm.data(), (size_t)L.quads * sizeof(int32_t));
    }
    return L.quads;
}

extern "C" int32_t dice_ctx_program_stage(const dice_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->kind == 1 && ctx->prog.mfma ? (ctx->prog.mfma_forced ? 2 : 1) : 0;
}

extern "C" int64_t dice_program_mfma_tables(const dice_templates* t, int32_t* dims, uint32_t* frag, int64_t frag_cap,
                                            int32_t* map, int64_t map_cap) {
    if (!t || t->n_templates < 1 || t->n_vocab < 1 || !t->lf_bits || t->n_templates > dice::kProgramMaxTemplates)
        return -1;
    dice::Program prog;
    (void)dice::compact_source_for(t, prog);
    const dice::MfmaTables& m = prog.mf;
    if (dims) {
        dims[0] = m.ksteps;
        dims[1] = m.ntiles;
        dims[2] = prog.layout.bit_dwords;
        dims[3] = m.pays ? 1 : 0;
    }
    if (!m.eligible) return 0;
    if (frag) {
        if (frag_cap < (int64_t)m.frag.size()) return -1;
        memcpy(frag, m.frag.data(), m.frag.size() * sizeof(uint32_t));
    }
    if (map) {
        if (map_cap < (int64_t)m.map.size()) return -1;
        memcpy(map, m.map.data(), m.map.size() * sizeof(int32_t));
    }
    return (int64_t)m.frag.size();
}

extern "C" int64_t dice_program_source(const dice_templates* t, char* buf, int64_t cap) {
    if (!t || t->n_templates < 1 || t->n_vocab < 1 || !t->lf_bits) return -1;
    dice::Program prog;
    const std::string src = dice::source_for(t, prog);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, src.size());
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return (int64_t)src.size();
}
