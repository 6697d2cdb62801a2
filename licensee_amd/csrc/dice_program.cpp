// Template-specialized sparse scoring program for small corpora (T <= 64), gfx950: the runtime side.
//
// The program's HIP source is generated per corpus by dice_program_gen.cpp (plan_program, then
// emit_program; the kernels and their design are described there). This file reads the switches
// from the environment, compiles the source with hiprtc for gfx950, caches the code object by hash
// under the library directory (lib/cache/dice_prog_<hash>.co), so a corpus compiles once per machine
// image, loads and launches the kernels, and holds the program's part of the C ABI.
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

// The switches, read at dice_create (program_setup) and by the exports, nowhere else.
// DICE_PROG_LAYOUT=bits keeps the full-bitset tile (fallback and A/B leg); DICE_PROG_MATCH=valu|mfma
// overrides the matrix-core cost rule; DICE_PROG_DIAG (diag_env: -DDICE_DIAG builds only) makes
// results wrong.
static ProgramOptions program_options_from_env() {
    ProgramOptions o;
    auto is = [](const char* v, const char* s) { return v && strcmp(v, s) == 0; };
    o.compact = !is(getenv("DICE_PROG_LAYOUT"), "bits");
    const char* pm = getenv("DICE_PROG_MATCH");
    o.match = is(pm, "mfma") ? ProgramOptions::kMfma : is(pm, "valu") ? ProgramOptions::kValu : ProgramOptions::kAuto;
    const char* diag = diag_env("DICE_PROG_DIAG");
    o.diag = is(diag, "noacc")    ? ProgramOptions::kNoAcc
             : is(diag, "noepi")  ? ProgramOptions::kNoEpi
             : is(diag, "timing") ? ProgramOptions::kTiming
             : is(diag, "nomfma") ? ProgramOptions::kNoMfma
                                  : ProgramOptions::kNone;
    return o;
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

// The matrix-core kernels take a launch when the module has them and the batch gives every CU a
// tile (below that the fragment fill per workgroup outweighs the stage; DICE_PROG_MATCH=mfma
// takes them at every size). One workgroup per CU at most, never more than there are tiles.
static bool mfma_launch(const dice_ctx* c, int64_t n_tiles, unsigned* grid) {
    if (!c->prog.mfma || !(c->prog.mfma_forced || n_tiles >= c->n_cu)) return false;
    *grid = (unsigned)std::min<int64_t>(n_tiles, c->n_cu);
    return true;
}

static bool program_wanted(const dice_templates* t) {
    const char* force = getenv("DICE_FORCE_DENSE");
    return !(force && *force == '1') && t->n_templates <= kProgramMaxTemplates;
}

int program_setup(dice_ctx* c, const dice_templates* t) {
    c->kind = 0;
    c->twq = c->wq;
    if (!program_wanted(t)) return DICE_OK;
    c->prog = plan_program(t, program_options_from_env());
    const Program& p = c->prog;
    std::vector<char> code;
    int rc = compile_cached(emit_program(t, p), code, nullptr);
    if (rc != DICE_OK) return rc;
    if (hipModuleLoadData(&c->module, code.data()) != hipSuccess) return fail(DICE_E_DEVICE, "hipModuleLoadData failed");
    auto get = [&](hipFunction_t* fn, const char* name) { return hipModuleGetFunction(fn, c->module, name) == hipSuccess; };
    if (!get(&c->prog_match, "dice_prog_match") || !get(&c->prog_matrix, "dice_prog_matrix4") ||
        !get(&c->prog_matrix16, "dice_prog_matrix16") || !get(&c->prog_topk, "dice_prog_topk4") ||
        !get(&c->prog_topk16, "dice_prog_topk16") ||
        (p.mfma && !get(&c->prog_match_mfma, "dice_prog_match_mfma")))
        return fail(DICE_E_DEVICE, "hipModuleGetFunction failed");
    if (p.sched.qperm.size() != (size_t)p.wq) return fail(DICE_E_STATE, "program tile permutation size");
    if (p.opts.compact) {   // the module's own dice_pack_compact fills the tile
        if (!get(&c->prog_pack, "dice_pack_compact")) return fail(DICE_E_DEVICE, "hipModuleGetFunction failed");
    } else {                // dice_pack_tiles (dice.hip) applies the permutation
        const size_t bytes = p.sched.qperm.size() * sizeof(int32_t);
        if ((rc = c->d_qperm.reserve(p.sched.qperm.size())) != DICE_OK) return rc;
        if (hipMemcpy(c->d_qperm, p.sched.qperm.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(DICE_E_DEVICE, "program tile permutation upload failed");
    }
    c->twq = p.wq;
    c->kind = 1;
    return DICE_OK;
}

int program_launch_pack(dice_ctx* c, dice_batch* b, int64_t n, hipStream_t s) {
    const int64_t n_tiles = (n + 63) / 64;
    if (n_tiles == 0) return DICE_OK;
    void* args[] = {b->d_rows.arg(), &n, b->d_tiles.arg()};
    if (hipModuleLaunchKernel(c->prog_pack, (unsigned)n_tiles, 1, 1, 256, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_pack_compact failed");
    return DICE_OK;
}

int program_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s) {
    const int64_t n_tiles = (b->n + 63) / 64;
    const int32_t wpb = kProgramWaves;
    unsigned grid = (unsigned)((n_tiles + wpb - 1) / wpb), threads = 64 * wpb;
    hipFunction_t fn = c->prog_match;
    if (mfma_launch(c, n_tiles, &grid)) {
        fn = c->prog_match_mfma;
        threads = 64 * kMfmaMatchWaves;
    }
    int64_t n = b->n;
    void* args[] = {b->d_tiles.arg(), &n, b->d_wf.arg(), b->d_len.arg(), b->d_cc.arg(), &thr, b->d_best.arg(),
                    b->d_ov.arg(), b->d_score.arg()};
    if (hipModuleLaunchKernel(fn, grid, 1, 1, threads, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_prog_match failed");
    return DICE_OK;
}

int program_launch_matrix(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s) {
    const int64_t n_tiles = (b->n + 63) / 64;
    const int32_t wpb = kProgramWaves;
    const unsigned grid = (unsigned)((n_tiles + wpb - 1) / wpb);
    int64_t n = b->n;
    int32_t kk = k;
    int32_t* tki = k > 0 ? b->d_tki.get() : nullptr;
    double* tks = k > 0 ? b->d_tks.get() : nullptr;
    void* args[] = {b->d_tiles.arg(), &n, b->d_wf.arg(), b->d_len.arg(), b->d_cc.arg(), &kk, b->d_mov.arg(),
                    b->d_mscore.arg(), &tki, &tks};
    hipFunction_t fn = k <= 4 ? c->prog_matrix : c->prog_matrix16;
    if (hipModuleLaunchKernel(fn, grid, 1, 1, 64 * wpb, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_prog_matrix failed");
    return DICE_OK;
}

int program_launch_topk(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s) {
    const int64_t n_tiles = (b->n + 63) / 64;
    const int32_t wpb = kProgramWaves;
    const unsigned grid = (unsigned)((n_tiles + wpb - 1) / wpb);
    int64_t n = b->n;
    int32_t kk = k;
    void* args[] = {b->d_tiles.arg(), &n, b->d_wf.arg(), b->d_len.arg(), b->d_cc.arg(), &kk, b->d_tki.arg(), b->d_tks.arg()};
    // the VALU program under every DICE_PROG_MATCH: the matrix-core stage measured slower here too
    // (DESIGN.md Appendix B), the k sorted slots' offers bound the kernel, not the accumulation
    hipFunction_t fn = k <= 4 ? c->prog_topk : c->prog_topk16;
    if (hipModuleLaunchKernel(fn, grid, 1, 1, 64 * wpb, 1, 1, 0, s, args, nullptr) != hipSuccess)
        return fail(DICE_E_DEVICE, "launch dice_prog_topk failed");
    return DICE_OK;
}

}  // namespace dice

static_assert(dice::kProgramMaxTemplates <= dice::kMaxIndexedTemplates, "the match kernels' index byte");

// The exports' argument check; `any_size` also takes corpora of more templates than the program serves.
static bool templates_ok(const dice_templates* t, bool any_size = false) {
    return t && t->n_templates >= 1 && t->n_vocab >= 1 && t->lf_bits && (any_size || t->n_templates <= dice::kProgramMaxTemplates);
}

// The plan for the environment's switches, with the layout given.
static dice::Program plan_from_env(const dice_templates* t, bool compact) {
    dice::ProgramOptions o = dice::program_options_from_env();
    o.compact = compact;
    return dice::plan_program(t, o);
}

// Its source, under the exports' buffer contract.
static int64_t source_out(const dice_templates* t, bool compact, char* buf, int64_t cap) {
    const std::string src = dice::emit_program(t, plan_from_env(t, compact));
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, src.size());
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return (int64_t)src.size();
}

extern "C" int dice_precompile(const dice_templates* t, char* path, int32_t path_cap) {
    if (!templates_ok(t, true)) return dice::fail(DICE_E_ARG, "invalid dice_templates");
    if (!dice::program_wanted(t)) return dice::fail(DICE_E_STATE, "corpus uses the dense kernel");
    // both layouts, so the DICE_PROG_LAYOUT=bits leg finds its code object too; the path
    // written is the one dice_create will load
    std::string p[2];
    for (int compact = 0; compact < 2; ++compact) {
        std::vector<char> code;
        int rc = dice::compile_cached(dice::emit_program(t, plan_from_env(t, compact != 0)), code, &p[compact]);
        if (rc != DICE_OK) return rc;
    }
    if (path && path_cap > 0)
        snprintf(path, (size_t)path_cap, "%s", p[dice::program_options_from_env().compact ? 1 : 0].c_str());
    return DICE_OK;
}

extern "C" int64_t dice_program_source(const dice_templates* t, char* buf, int64_t cap) {
    return templates_ok(t, true) ? source_out(t, false, buf, cap) : -1;
}

extern "C" int64_t dice_program_source_compact(const dice_templates* t, char* buf, int64_t cap) {
    return templates_ok(t) ? source_out(t, true, buf, cap) : -1;
}

extern "C" int32_t dice_program_layout(const dice_templates* t, int32_t* dest, int32_t* count_base, int32_t* qperm,
                                       int32_t qperm_cap) {
    if (!templates_ok(t)) return -1;
    const dice::Program prog = plan_from_env(t, true);
    const dice::CompactLayout& L = prog.layout;
    if (dest) memcpy(dest, L.dest.data(), L.dest.size() * sizeof(int32_t));
    if (count_base) *count_base = 4 * L.bit_dwords;
    if (qperm) {
        if (qperm_cap < L.quads) return -1;
        memcpy(qperm, prog.sched.qperm.data(), (size_t)L.quads * sizeof(int32_t));
    }
    return L.quads;
}

extern "C" int32_t dice_ctx_program_stage(const dice_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->kind == 1 && ctx->prog.mfma ? (ctx->prog.mfma_forced ? 2 : 1) : 0;
}

extern "C" int64_t dice_program_mfma_tables(const dice_templates* t, int32_t* dims, uint32_t* frag, int64_t frag_cap,
                                            int32_t* map, int64_t map_cap) {
    if (!templates_ok(t)) return -1;
    const dice::Program prog = plan_from_env(t, true);
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

extern "C" int32_t dice_program_mfma_rows(const dice_templates* t, int32_t* rows, uint8_t* live, int64_t live_cap) {
    if (!templates_ok(t)) return -1;
    const dice::Program prog = plan_from_env(t, true);
    const dice::MfmaTables& m = prog.mf;
    if (!m.eligible) return 0;
    if (rows) {
        for (int i = 0; i < 64; ++i) rows[i] = i < (int)m.rows.size() ? m.rows[(size_t)i] : -1;
    }
    if (live) {
        if (live_cap < (int64_t)m.live.size()) return -1;
        memcpy(live, m.live.data(), m.live.size());
    }
    return m.n_live;
}
